"""Writes tests/golden/abi_table_parent.json: the ctypes binding of pcp_amd/lib.py as plain data.

    python tests/golden/make_abi_table.py

The committed file was written by the commit that still kept lib.py as a hand-written mirror of include/*.h; tests/test_abi_binding_cpu.py
pins the binding derived from the headers to it.  Only lib's public tables are read (SYMBOLS, the struct classes, the integer constants,
OPTIONS, _OPTION_ENV), so the script runs unchanged on either form of lib.py.

  symbols   name -> [restype, [argtypes]] as ABI classes: i32 u32 i64 u64 f32 f64 cstr ptr, or ptr:<C struct name>
  structs   Python name -> {c_name, size, fields: [[name, offset, class, array length | null, embedded C struct | null]]}
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))

# Python class of lib.py -> struct of the headers, stated here on its own
STRUCTS = {
    'Grid': 'pcp_grid_t', 'Conv3x3': 'pcp_conv3x3_t', 'Pointwise': 'pcp_pointwise_t', 'Decode': 'pcp_decode_t', 'DetHead': 'pcp_det_head_t',
    'Anchor': 'pcp_anchor_t', 'DecodeHead': 'pcp_decode_head_t', 'DetHeadExt': 'pcp_det_head_ext_t', 'RowMap': 'pcp_rowmap_t',
    'Target': 'pcp_target_t', 'HeadLoss': 'pcp_headloss_t', 'TargetHead': 'pcp_target_head_t', 'HeadLossHead': 'pcp_headloss_head_t',
    'HeadLossExt': 'pcp_headloss_ext_t', 'AnchorAssign': 'pcp_anchor_assign_t', 'AnchorLoss': 'pcp_anchor_loss_t',
    'HunterMeta': 'pcp_hunter_meta_t', 'HunterLoss': 'pcp_hunter_loss_t', 'PackJob': 'pcp_pack_job_t', 'WorldAug': 'pcp_world_aug_t',
    'ObjectAug': 'pcp_object_aug_t', 'MpConv3x3': 'pcp_mp_conv3x3_t', 'MpPackJob': 'pcp_mp_pack_job_t', 'MpWgrad3x3': 'pcp_mp_wgrad3x3_t',
    'MpPointwise': 'pcp_mp_pointwise_t', 'MpRowMap': 'pcp_mp_rowmap_t',
}

_CODES = {'f': 'f32', 'd': 'f64', 'z': 'cstr', 'P': 'ptr'}


def abi_class(t, c_names):
    """c_names: struct class -> C name"""
    if hasattr(t, 'contents'):                                  # POINTER(...)
        return 'ptr:' + c_names[t._type_] if t._type_ in c_names else 'ptr'
    code = t._type_
    if code in _CODES:
        return _CODES[code]
    assert code in 'iIlLqQ', t
    return ('i' if code.islower() else 'u') + str(8 * ctypes.sizeof(t))


def table(lib):
    """lib: the module, or any object with its public names"""
    c_names = {getattr(lib, py): c for py, c in STRUCTS.items()}
    structs = {}
    for py, c in STRUCTS.items():
        cls, fields = getattr(lib, py), []
        for name, t in cls._fields_:
            length = None
            if hasattr(t, '_length_'):
                t, length = t._type_, t._length_
            embedded = c_names.get(t)
            fields.append([name, getattr(cls, name).offset, 'struct' if embedded else abi_class(t, c_names), length, embedded])
        structs[py] = {'c_name': c, 'size': ctypes.sizeof(cls), 'fields': fields}
    symbols = {name: [abi_class(res, c_names), [abi_class(a, c_names) for a in args]] for name, (res, args) in lib.SYMBOLS.items()}
    constants = {k: v for k, v in vars(lib).items() if k.isupper() and not k.startswith('_') and type(v) is int}
    return {'symbols': symbols, 'structs': structs, 'constants': constants, 'options': dict(lib.OPTIONS), 'option_env': dict(lib._OPTION_ENV)}


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(REPO, 'practical-collab-perception_amd'))
    from pcp_amd import lib
    with open(os.path.join(HERE, 'abi_table_parent.json'), 'w') as f:
        json.dump(table(lib), f, indent=1, sort_keys=True)
        f.write('\n')
