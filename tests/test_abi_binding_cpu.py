"""The ctypes binding of pcp_amd/lib.py is derived from include/*.h (pcp_amd/abi_header.py).  CPU-only checks of that derivation:
it equals the hand-written binding of the commit before it (tests/golden/abi_table_parent.json, written by that commit through
tests/golden/make_abi_table.py), it covers every struct and prototype of the headers, the C compiler agrees with ctypes about every
struct's size and field offsets, the reader refuses what is outside the headers' dialect, a deliberate fault in a header changes the
derived table, and c_void_p takes every kind of host argument the call sites pass."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import types

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(REPO, 'tests', 'golden'))

import make_abi_table  # noqa: E402
from pcp_amd import abi_header, lib  # noqa: E402

HEADER_PATHS = [os.path.join(REPO, 'include', h) for h in lib.HEADERS]
with open(os.path.join(REPO, 'tests', 'golden', 'abi_table_parent.json')) as _f:
    PARENT = json.load(_f)


def derived_table(headers):
    """the binding lib.py derives from `headers`, in the fixture's form"""
    return json.loads(json.dumps(make_abi_table.table(types.SimpleNamespace(**lib.derive(headers)))))


def changed_since_parent(table):
    """every recorded entry `table` does not hold identically (entries the parent did not have are no change)"""
    return ['%s/%s' % (section, name) for section, entries in PARENT.items() for name, value in entries.items()
            if table[section].get(name) != value]


def test_the_derived_binding_equals_the_parents_hand_written_one():
    assert len(PARENT['symbols']) == 200 and len(PARENT['structs']) == 26 and len(PARENT['constants']) == 51
    assert len(PARENT['options']) == 9 and len(PARENT['option_env']) == 9
    assert changed_since_parent(derived_table(HEADER_PATHS)) == []
    # and the module's own names are that derivation
    assert changed_since_parent(json.loads(json.dumps(make_abi_table.table(lib)))) == []


def test_every_struct_and_prototype_of_the_headers_is_bound():
    text = ''.join(open(p).read() for p in HEADER_PATHS)
    assert sorted(os.listdir(os.path.join(REPO, 'include'))) == sorted(lib.HEADERS)
    typedefs = re.findall(r'^\}\s*(\w+)\s*;', text, flags=re.M)
    assert len(typedefs) == text.count('typedef struct') == 26
    assert sorted(lib.STRUCT_NAMES.values()) == sorted(typedefs)                    # every struct under exactly one Python name
    classes = [getattr(lib, py) for py in lib.STRUCT_NAMES]
    assert len(set(classes)) == len(classes) and all(issubclass(c, ctypes.Structure) for c in classes)
    assert lib.STRUCT_NAMES == make_abi_table.STRUCTS                               # the generator states the names on its own
    declared = set(re.findall(r'\b(pcp_[a-z0-9_]+)\s*\(', text))
    assert declared == set(lib.SYMBOLS) and len(declared) >= 200
    consts = set(re.findall(r'#define\s+PCP_(\w+)[ \t]+\d', text)) | set(re.findall(r'^\s*PCP_(\w+)\s*=\s*\d', text, flags=re.M))
    assert consts and all(isinstance(getattr(lib, c), int) for c in consts)
    assert lib.OPTIONS == {k[4:].lower(): getattr(lib, k) for k in consts if k.startswith('OPT_') and k != 'OPT_COUNT'}
    assert len(lib.OPTIONS) == lib.OPT_COUNT and lib.ABI_VERSION == 1 and lib.ERR_ARG == 1


def _c_compiler():
    for cc in ('cc', 'clang', os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin', 'clang')):
        if shutil.which(cc):
            return shutil.which(cc)
    return None


def test_the_c_compiler_agrees_about_every_struct_size_and_field_offset(tmp_path):
    """independent of the header reader: only the struct and field NAMES come from the derived classes"""
    cc = _c_compiler()
    if cc is None:
        pytest.skip('no host C compiler (cc, clang or the ROCm clang)')
    src = ['#include <stdio.h>', '#include <stddef.h>'] + ['#include "%s"' % h for h in lib.HEADERS] + ['int main(void) {']
    want = []
    for py, c in lib.STRUCT_NAMES.items():
        cls = getattr(lib, py)
        src.append('  printf("%s %%lu\\n", (unsigned long) sizeof(%s));' % (c, c))
        want.append('%s %d' % (c, ctypes.sizeof(cls)))
        for name, _t in cls._fields_:
            src.append('  printf("%s.%s %%lu %%lu\\n", (unsigned long) offsetof(%s, %s), (unsigned long) sizeof(((%s *) 0)->%s));'
                       % (c, name, c, name, c, name))
            want.append('%s.%s %d %d' % (c, name, getattr(cls, name).offset, getattr(cls, name).size))
    src += ['  return 0;', '}', '']
    (tmp_path / 'abi_probe.c').write_text('\n'.join(src))
    exe = str(tmp_path / 'abi_probe')
    subprocess.check_call([cc, '-std=c99', '-Wall', '-pedantic', '-I', os.path.join(REPO, 'include'), str(tmp_path / 'abi_probe.c'), '-o', exe])
    got = subprocess.check_output([exe]).decode().split('\n')[:-1]
    assert len(want) > 26 * 3
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:10]


OK_STRUCT = 'typedef struct { int32_t a; } pcp_a_t;\n'
REFUSED = {
    'unknown type name': 'int pcp_f(uint16_t x);',
    'unknown type behind a pointer': 'int pcp_f(const foo_t *x);',
    'unnamed parameter': 'int pcp_f(int32_t a, float);',
    'unnamed pointer parameter': 'int pcp_f(const float *);',
    'function pointer parameter': 'int pcp_f(void (*done)(int32_t status), void *stream);',
    'function pointer field': 'typedef struct { void (*done)(void); } pcp_b_t;',
    'bit-field': 'typedef struct { int32_t a : 3; } pcp_b_t;',
    'union': 'typedef union { int32_t a; float b; } pcp_b_t;',
    'union in a struct': 'typedef struct { union { int32_t a; float b; } u; } pcp_b_t;',
    'array parameter': 'int pcp_f(const float theta[6], void *stream);',
    'define that is no integer literal': '#define PCP_SCALE 1.5f',
    'define that is an expression': '#define PCP_TWICE (2 * PCP_ONCE)',
    'function-like define': '#define PCP_MIN(a, b) ((a) < (b) ? (a) : (b))',
    'constant declared twice': '#define PCP_N 4\n#define PCP_N 4',
    'enumerator declared twice': '#define PCP_N 4\nenum { PCP_N = 4 };',
    'function declared twice': 'int pcp_f(int32_t a);\nint pcp_f(int32_t a);',
    'struct declared twice': OK_STRUCT + OK_STRUCT,
    'field declared twice': 'typedef struct { int32_t a, b; float a; } pcp_b_t;',
    'struct used before it is declared': 'int pcp_f(const pcp_a_t *desc);\n' + OK_STRUCT,
    'struct embedded before it is declared': 'typedef struct { pcp_a_t a; } pcp_b_t;\n' + OK_STRUCT,
    'array length that is no earlier constant': 'typedef struct { int32_t a[PCP_N]; } pcp_b_t;\n#define PCP_N 4',
    'scalar type by value that the rule does not name': 'int pcp_f(uint8_t flag);',
    'struct by value in a prototype': OK_STRUCT + 'int pcp_f(pcp_a_t desc);',
    'pointer return type': 'float *pcp_f(int32_t n);',
    'enumerator without a value': 'enum { PCP_A, PCP_B };',
    'named enum': 'enum pcp_mode { PCP_A = 0 };',
    'variadic prototype': 'int pcp_f(const char *fmt, ...);',
    'unsigned int': 'int pcp_f(unsigned int n);',
}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_the_reader_refuses(what):
    with pytest.raises(abi_header.PcpError) as e:
        abi_header.read([('synthetic.h', '#include <stdint.h>\n' + REFUSED[what] + '\n')])
    assert str(e.value).startswith('synthetic.h: ')          # the header, then the declaration
    assert '`' in str(e.value)


def test_the_reader_takes_the_dialect():
    abi = abi_header.read([('synthetic.h', '''
        #ifndef PCP_SYNTHETIC_H
        #define PCP_SYNTHETIC_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define PCP_N 4u   /* a comment; with a semicolon */
        enum { PCP_A = 0, PCP_B = 0x10 };  // and another
        typedef struct pcp_a { int32_t x, y[PCP_N]; const float *p, *q; uint64_t big; float lim[6]; } pcp_a_t;
        typedef struct { pcp_a_t a; int64_t n; } pcp_b_t;
        const char *pcp_name(int status);
        size_t pcp_bytes(const pcp_b_t *desc,
                         int64_t n);
        int pcp_run(const pcp_a_t *a, const void *const *maps_host, double *flops, uint8_t *mask, uint32_t flags, float s, void *stream);
        int pcp_none(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
        ''')])
    assert abi.constants == {'PCP_N': 4, 'PCP_A': 0, 'PCP_B': 16}
    a, b = abi.structs['pcp_a_t'], abi.structs['pcp_b_t']
    assert [(n, t) for n, t in a._fields_] == [('x', ctypes.c_int32), ('y', ctypes.c_int32 * 4), ('p', ctypes.c_void_p), ('q', ctypes.c_void_p),
                                               ('big', ctypes.c_uint64), ('lim', ctypes.c_float * 6)]
    assert b._fields_ == [('a', a), ('n', ctypes.c_int64)]
    assert abi.prototypes == {
        'pcp_name': (ctypes.c_char_p, [ctypes.c_int32]),
        'pcp_bytes': (ctypes.c_size_t, [ctypes.POINTER(b), ctypes.c_int64]),
        'pcp_run': (ctypes.c_int32, [ctypes.POINTER(a), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float,
                                     ctypes.c_void_p]),
        'pcp_none': (ctypes.c_int32, []),
    }


def _swap_dhead(text):
    return re.subn(r'(  float \*dhead;[^\n]*\n)(  int32_t ld_dhead;\n)', r'\2\1', text)


FAULTS = {
    # what: (header, edit -> (text, replacements), the recorded entries that must change)
    'int32_t to int64_t in an argument of pcp_hunter_point_head_ex':
        ('pcp_hip.h', lambda t: (t.replace('int32_t apply_flow,\n', 'int64_t apply_flow,\n'), t.count('int32_t apply_flow,\n')),
         ['symbols/pcp_hunter_point_head_ex']),
    'an argument removed from pcp_sc_gate_backward':
        ('pcp_hip_train.h', lambda t: (t.replace('int32_t accumulate_dx, float *ds,', 'float *ds,'), t.count('int32_t accumulate_dx, float *ds,')),
         ['symbols/pcp_sc_gate_backward']),
    'two fields of pcp_hunter_loss_t swapped': ('pcp_hip_train.h', _swap_dhead, ['structs/HunterLoss']),
    'PCP_TGT_MAX_CLASSES changed':
        ('pcp_hip_train.h', lambda t: (t.replace('#define PCP_TGT_MAX_CLASSES 32\n', '#define PCP_TGT_MAX_CLASSES 16\n'),
                                       t.count('#define PCP_TGT_MAX_CLASSES 32\n')),
         ['structs/TargetHead', 'constants/TGT_MAX_CLASSES']),
}


@pytest.mark.parametrize('what', sorted(FAULTS))
def test_a_fault_in_a_header_fails_the_parent_pin(what, tmp_path):
    header, edit, must_change = FAULTS[what]
    paths = []
    for p in HEADER_PATHS:
        text = open(p).read()
        if os.path.basename(p) == header:
            text, n = edit(text)
            assert n == 1, 'the edit no longer finds its place in %s' % header
        paths.append(str(tmp_path / os.path.basename(p)))
        with open(paths[-1], 'w') as f:
            f.write(text)
    assert sorted(changed_since_parent(derived_table(paths))) == sorted(must_change)


def test_c_void_p_takes_every_kind_of_host_argument_the_call_sites_pass():
    """the header does not say which pointers are host memory, so all of them are c_void_p: what ops.py, train_ops.py and det_eval.py hand
    to such an argument must still convert, and to the object's own address"""
    np = pytest.importorskip('numpy')
    conv = ctypes.c_void_p.from_param
    i, f, d, z = ctypes.c_int32(7), ctypes.c_float(1.5), ctypes.c_double(2.5), ctypes.c_size_t(9)
    for obj in (i, f, d, z):
        assert conv(ctypes.byref(obj)) is not None
        assert ctypes.cast(conv(ctypes.pointer(obj)), ctypes.c_void_p).value == ctypes.addressof(obj)
    for arr in ((ctypes.c_float * 6)(*range(6)), (ctypes.c_int32 * 3)(1, 2, 3), (ctypes.c_void_p * 2)(16, 32), (ctypes.c_uint8 * 4)(1, 0, 1, 0)):
        assert ctypes.cast(conv(arr), ctypes.c_void_p).value == ctypes.addressof(arr)
    assert conv(None) is None                                  # NULL
    assert conv(ctypes.c_void_p(4096)).value == 4096           # a device address (_p(tensor), _stream())
    assert conv(4096) is not None
    for a, t in ((np.arange(6, dtype=np.float32), ctypes.c_float), (np.arange(12, dtype=np.float64), ctypes.c_double),
                 (np.ones(4, dtype=np.uint8), ctypes.c_uint8)):
        assert ctypes.cast(conv(a.ctypes.data_as(ctypes.POINTER(t))), ctypes.c_void_p).value == a.ctypes.data
    # and through a real call: memcpy of libc bound the way SYMBOLS binds a host pointer
    memcpy = ctypes.CDLL(None).memcpy
    memcpy.restype, memcpy.argtypes = ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    dst, out = (ctypes.c_float * 6)(), ctypes.c_double(0)
    memcpy(dst, np.arange(6, dtype=np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 24)
    memcpy(ctypes.byref(out), ctypes.byref(d), 8)
    assert list(dst) == [0, 1, 2, 3, 4, 5] and out.value == 2.5
    # the struct descriptors keep their own type: a wrong struct is refused before the call
    assert lib.SYMBOLS['pcp_conv3x3'][1][0] is ctypes.POINTER(lib.Conv3x3)
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        ctypes.POINTER(lib.Conv3x3).from_param(ctypes.byref(lib.Grid()))
