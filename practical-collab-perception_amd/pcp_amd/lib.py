"""ctypes binding of libpcp_hip.so, derived from the C headers (include/pcp_hip.h, pcp_hip_train.h, pcp_hip_mp.h) when it is imported.

The headers are the only statement of the ABI: abi_header.py reads them, and every prototype becomes an entry of SYMBOLS, every struct a
ctypes.Structure under its Python name of STRUCT_NAMES (fields in the header's order), every PCP_X constant the module attribute X.
The library is built in-tree by `make -C practical-collab-perception_amd/csrc` (or __graft_entry__.build()).  There is NO
fallback: if a header or the shared object is missing or a symbol cannot be resolved the import of the product path fails loudly.
"""
import ctypes
import os

from . import abi_header
from .abi_header import PcpError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PCP_HIP_LIB') or os.path.abspath(os.path.join(_HERE, '..', 'lib', 'libpcp_hip.so'))   # override: kernel A/B builds
INCLUDE_DIR = os.path.abspath(os.path.join(_HERE, '..', '..', 'include'))
HEADERS = ('pcp_hip.h', 'pcp_hip_train.h', 'pcp_hip_mp.h')       # in dependency order

# Python name of every struct of the headers (the names follow no one spelling rule)
STRUCT_NAMES = {
    'Grid': 'pcp_grid_t',
    'Conv3x3': 'pcp_conv3x3_t',
    'Pointwise': 'pcp_pointwise_t',
    'Decode': 'pcp_decode_t',
    'DetHead': 'pcp_det_head_t',
    'Anchor': 'pcp_anchor_t',
    'DecodeHead': 'pcp_decode_head_t',
    'DetHeadExt': 'pcp_det_head_ext_t',
    'RowMap': 'pcp_rowmap_t',
    'Target': 'pcp_target_t',
    'HeadLoss': 'pcp_headloss_t',
    'TargetHead': 'pcp_target_head_t',
    'HeadLossHead': 'pcp_headloss_head_t',
    'HeadLossExt': 'pcp_headloss_ext_t',
    'AnchorAssign': 'pcp_anchor_assign_t',
    'AnchorLoss': 'pcp_anchor_loss_t',
    'HunterMeta': 'pcp_hunter_meta_t',
    'HunterLoss': 'pcp_hunter_loss_t',
    'PackJob': 'pcp_pack_job_t',
    'WorldAug': 'pcp_world_aug_t',
    'ObjectAug': 'pcp_object_aug_t',
    'MpConv3x3': 'pcp_mp_conv3x3_t',
    'MpPackJob': 'pcp_mp_pack_job_t',
    'MpWgrad3x3': 'pcp_mp_wgrad3x3_t',
    'MpPointwise': 'pcp_mp_pointwise_t',
    'MpRowMap': 'pcp_mp_rowmap_t',
}

# Job tables that live in DEVICE memory (pcp_pack_conv3x3_group, pcp_mp_pack_conv3x3_group take the table's address): a pointer to one of
# these is bound as c_void_p, every other struct pointer as POINTER(struct)
DEVICE_TABLE_STRUCTS = ('pcp_pack_job_t', 'pcp_mp_pack_job_t')


def derive(headers):
    """every public name the headers give this module, as a dict: SYMBOLS name -> (restype, argtypes), the struct classes, the constants,
    OPTIONS (the PCP_OPT_* enumerators) and _OPTION_ENV (the environment variable of each option)"""
    abi = abi_header.read(headers, address_only=DEVICE_TABLE_STRUCTS)
    unnamed = set(abi.structs) - set(STRUCT_NAMES.values())
    missing = set(STRUCT_NAMES.values()) - set(abi.structs)
    if unnamed or missing:
        raise PcpError('lib.STRUCT_NAMES and the headers disagree: no Python name for %s, no declaration of %s'
                       % (sorted(unnamed) or 'none', sorted(missing) or 'none'))
    names = {c[len('PCP_'):]: v for c, v in abi.constants.items()}
    names.update((py, abi.structs[c]) for py, c in STRUCT_NAMES.items())
    names['SYMBOLS'] = abi.prototypes
    # The C library never reads the environment; the PCP_* variables of earlier rounds are mapped onto the option table ONCE, when the
    # library is loaded (set_option() changes an option later, e.g. from a test)
    names['OPTIONS'] = {c[len('PCP_OPT_'):].lower(): v for c, v in abi.constants.items() if c.startswith('PCP_OPT_') and c != 'PCP_OPT_COUNT'}
    names['_OPTION_ENV'] = {'PCP_' + name.upper(): name for name in names['OPTIONS']}
    return names


_paths = [os.path.join(INCLUDE_DIR, h) for h in HEADERS]
for _p in _paths:
    if not os.path.isfile(_p):
        raise PcpError('header %s not found -- the ctypes binding is derived from include/*.h of the source tree; there is no second '
                       'copy of the ABI to fall back on.' % _p)
globals().update(derive(_paths))


def check_gt_box_width(width, what='gt_boxes'):
    """the refusal of the HunterJr training kernels, on the host and before any launch"""
    if not GT_BOX_MIN_WIDTH <= int(width) <= GT_BOX_MAX_WIDTH:
        raise ValueError('%s rows have %d columns: the HunterJr training kernels take %d (x y z dx dy dz heading class) up to %d, the '
                         'number of box codes the head kernels take' % (what, int(width), GT_BOX_MIN_WIDTH, GT_BOX_MAX_WIDTH))
    return int(width)


_LIB = None


def load():
    """dlopen the library once; raises (never falls back) when it is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.isfile(LIB_PATH):
        raise PcpError('libpcp_hip.so not found at %s -- build it with `make -C practical-collab-perception_amd/csrc` '
                       '(or python -c "import __graft_entry__ as g; g.build()"); there is no CPU fallback.' % LIB_PATH)
    import torch  # noqa: F401  -- makes sure torch's own libamdhip64 (same SONAME) is the HIP runtime both sides use
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing: loud by design
        fn.restype = res
        fn.argtypes = args
    if lib.pcp_abi_version() != ABI_VERSION:
        raise PcpError('libpcp_hip.so ABI version mismatch')
    for env, name in _OPTION_ENV.items():
        v = os.environ.get(env, '')
        if v.strip():
            if lib.pcp_set_option(OPTIONS[name], int(v)) != 0:
                raise PcpError('%s=%s: pcp_set_option refused it' % (env, v))
    _LIB = lib
    return lib


def set_option(name, value):
    """override a built-in launch rule of the library (A/B runs, tests); value None restores the rule.  Returns the previous override (None = rule)."""
    lib = load()
    prev = int(lib.pcp_get_option(OPTIONS[name]))
    check(lib.pcp_set_option(OPTIONS[name], -1 if value is None else int(value)), 'pcp_set_option')
    return None if prev < 0 else prev


def check(status, what):
    if status != 0:
        raise PcpError('%s failed: %s' % (what, load().pcp_status_string(status).decode()))
