"""Recorder of the SECOND ops' host side: tests/golden/second_ops_calls.json.

Which C symbol a wrapper of the SECOND section of `pcp_amd.ops` calls, with which scalars, on which buffers of which size, what it reads
back and which exception it raises with which text are host-side decisions, so they are recorded on the CPU through the public surface
only.  For the duration of a case three names are replaced: `ops._need_cuda` notes the tensors it was asked about (its place among the
checks is part of the row), `ops._stream` returns a null handle, and `pcp_amd.lib.load` returns a fake library.  The fake records every
call and returns 0; a `*_bytes` symbol returns a scripted size (0: the "unsupported grid" refusals), and pcp_mean_vfe,
pcp_spconv_table_build and pcp_spconv_strided_sites write scripted counter words through the pointer they are handed.

Per C call a row holds the symbol, every integer, every int32[3] array as a list, and per pointer the role of the caller's tensor it points
into with its byte offset ('status+16'), 'null', or 'internal'; a buffer of the call's DevBuffers is a caller's tensor ('bufs.NAME').  Per op
call it holds dtype, shape and place of every returned tensor, a table's shape4 / capacity, the {name: (dtype, numel)} of the DevBuffers, the
number of host reads that start in a frame of a pcp_amd module, and an exception's type and exact text.
tests/test_second_ops_calls_cpu.py runs `record()` again and demands equality with the committed file on every row.

    python tests/golden/make_second_ops_calls.py          # rewrites the JSON; the file names the commit it was recorded at
"""
import contextlib
import ctypes
import json
import os
import subprocess
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _path in (REPO, os.path.join(REPO, 'practical-collab-perception_amd')):
    if _path not in sys.path:
        sys.path.insert(0, _path)
TABLE = os.path.join(HERE, 'second_ops_calls.json')

COUNTS = (0, 1, 17)
SHAPE4 = (2, 9, 24, 28)                                   # tests/test_gpu_spconv_devcount.py: SHAPE4
GEOMS = {'s2': ((3, 3, 3), (2, 2, 2), (1, 1, 1)), 'down': ((3, 1, 1), (2, 1, 1), (0, 0, 0))}      # the same file's GEOMS
VFE_RANGE, VFE_VOXEL, VFE_GRID = [0.0, 0.0, 0.0, 5.6, 4.8, 4.0], [0.1, 0.1, 0.1], [56, 48, 40]
_DT = {torch.float32: 'f32', torch.float64: 'f64', torch.float16: 'f16', torch.int32: 'i32', torch.int64: 'i64', torch.uint8: 'u8'}
READS = ('cpu', 'item', 'tolist', 'numpy')
# where each scripted symbol finds the counters it writes (argument index)
COUNTERS_AT = {'pcp_mean_vfe': 8, 'pcp_spconv_table_build': 9, 'pcp_spconv_strided_sites': 11}


def _table_bytes(B, D, H, W):
    return 64 + 8 * ((B * D * H * W + 63) // 64)


class Recorder:
    def __init__(self):
        self.named = []             # (role, tensor): the caller's tensors of the running case, kept alive
        self.bufs = None            # the DevBuffers of the running case
        self.calls = []
        self.reads = 0
        self.script = {}

    def begin(self, named, bufs, script):
        self.named, self.bufs, self.script = [(r, t) for r, t in named.items() if t is not None], bufs, dict(script)
        self.calls, self.reads = [], 0

    def _candidates(self):
        for role, t in self.named:
            yield role, t
        if self.bufs is not None:
            for name in sorted(self.bufs._t):
                yield 'bufs.' + name, self.bufs._t[name]

    def place(self, p):
        """the role of the named tensor the address lies in, with the byte offset"""
        if not p:
            return 'null'
        for role, t in self._candidates():
            base = t.data_ptr()
            if base and base <= p < base + max(t.numel() * t.element_size(), 1):
                return role if p == base else '%s+%d' % (role, p - base)
        return 'internal'

    def arg(self, v):
        if isinstance(v, bool) or v is None:
            return str(v)
        if isinstance(v, int):
            return v
        if isinstance(v, ctypes.c_void_p):
            return self.place(v.value)
        if isinstance(v, ctypes.Array):
            return [int(x) for x in v]
        if hasattr(v, '_obj'):          # ctypes.byref(grid)
            return 'byref(%s)' % type(v._obj).__name__
        return type(v).__name__

    def tensor(self, t):
        return '%s%s@%s' % (_DT.get(t.dtype, str(t.dtype)), list(t.shape), self.place(t.data_ptr()) if t.numel() else 'empty')

    def value(self, v):
        from pcp_amd import ops
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, ops.SpconvTable):
            return {'shape4': list(v.shape4), 'capacity': v.capacity, 'mem': self.value(v.mem), 'perm': self.value(v.perm)}
        if isinstance(v, (tuple, list)):
            return [self.value(u) for u in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return type(v).__name__

    def bufs_state(self):
        if self.bufs is None:
            return None
        return {name: [_DT.get(t.dtype, str(t.dtype)), int(t.numel())] for name, t in sorted(self.bufs._t.items())}


class FakeLib:
    """every symbol answers: noted with its arguments, scripted sizes and counter words, status 0"""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, sym):
        rec = self._rec

        def call(*a):
            rec.calls.append([sym] + [rec.arg(v) for v in a])
            if sym.endswith('_bytes'):
                size = rec.script.get(sym)
                if callable(size):
                    size = size(*a)
                if size is not None:
                    return size
                return _table_bytes(*a) if sym == 'pcp_spconv_table_bytes' else 1024 + 16 * a[-1]
            if sym in COUNTERS_AT:
                n = a[1]
                words = rec.script.get(sym)
                if words is None:
                    words = {'pcp_mean_vfe': ((n + 1) // 2, 0), 'pcp_spconv_table_build': (n, 0), 'pcp_spconv_strided_sites': ((n + 1) // 2,)}[sym]
                out = ctypes.cast(a[COUNTERS_AT[sym]], ctypes.POINTER(ctypes.c_int32))
                for i, w in enumerate(words):
                    out[i] = int(w)
            return 0
        return call


@contextlib.contextmanager
def _fakes(rec):
    from pcp_amd import lib, ops
    saved = [(ops, '_need_cuda', ops._need_cuda), (ops, '_stream', ops._stream), (lib, 'load', lib.load)]
    saved += [(torch.Tensor, name, getattr(torch.Tensor, name)) for name in READS]
    fake = FakeLib(rec)

    def need_cuda(*tensors):
        rec.calls.append(['_need_cuda'] + [rec.place(t.data_ptr()) if t is not None and t.numel() else str(t is not None) for t in tensors])

    def reader(orig):
        def wrapped(t, *a, **k):
            if sys._getframe(1).f_globals.get('__name__', '').startswith('pcp_amd.'):
                rec.reads += 1
            return orig(t, *a, **k)
        return wrapped
    ops._need_cuda, ops._stream, lib.load = need_cuda, (lambda: ctypes.c_void_p(0)), (lambda: fake)
    for name in READS:
        setattr(torch.Tensor, name, reader(getattr(torch.Tensor, name)))
    try:
        yield
    finally:
        for owner, name, fn in saved:
            setattr(owner, name, fn)


def _run(rec, fn, a=(), k=None, named=None, bufs=None, script=None, after=None):
    """one op call under the fakes -> its row"""
    k = dict(k or {})
    if bufs is not None:
        k['bufs'] = bufs
    rec.begin(named or {}, bufs, script or {})
    row = {}
    with _fakes(rec):
        try:
            out = fn(*a, **k)
            row['returns'] = rec.value(out)
            if after is not None:
                row.update(after(out))
        except Exception as e:                            # the type and the exact text are the row
            row['raises'] = [type(e).__name__, str(e)]
    row['calls'], row['reads'] = rec.calls, rec.reads
    if bufs is not None:
        row['bufs'] = rec.bufs_state()
    return row


def _twice(rec, rows, key, fn, a, k, named):
    """bufs=None, then one DevBuffers used twice: the second call's state must be the first's (it is part of the row either way)"""
    from pcp_amd import ops
    rows[key + ' bufs=None'] = _run(rec, fn, a, k, named)
    bufs = ops.DevBuffers()
    for i in (1, 2):
        rows['%s bufs call %d' % (key, i)] = _run(rec, fn, a, k, named, bufs=bufs)


def _points(n, cols=6, dtype=torch.float32):
    return torch.zeros((n, cols), dtype=dtype)


def _coords(n):
    return torch.zeros((n, 4), dtype=torch.int32)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _host_table(ops, n, shape4=SHAPE4, perm=True):
    return ops.SpconvTable(shape4, torch.zeros(_table_bytes(*shape4), dtype=torch.uint8), torch.zeros((max(n, 1),), dtype=torch.int32) if perm else None)


def _named_table(t):
    return {'table.mem': t.mem, 'table.perm': t.perm}


def _mean_vfe_rows(rec, ops, rows):
    grid = ops.make_grid(VFE_RANGE, VFE_VOXEL, VFE_GRID, 2)
    nz = VFE_GRID[2]
    for n in COUNTS:
        pts = _points(n)
        rows['mean_vfe n=%d' % n] = _run(rec, ops.mean_vfe, (pts, grid, 5), {'nz': nz}, {'points': pts})
        _twice(rec, rows, 'mean_vfe_dev n=%d' % n, ops.mean_vfe_dev, (pts, grid, 5), {'nz': nz}, {'points': pts})
    pts = _points(17, 9)
    for size in (16, 1 << 16):                            # a workspace too small (replaced) and one large enough (kept)
        ws = torch.zeros(size, dtype=torch.uint8)
        rows['mean_vfe workspace of %d bytes, 3 of 8 columns' % size] = _run(rec, ops.mean_vfe, (pts, grid, 3), {'nz': nz, 'workspace': ws},
                                                                             {'points': pts, 'workspace': ws})
    rows['mean_vfe_dev 3 of 8 columns'] = _run(rec, ops.mean_vfe_dev, (pts, grid, 3), {'nz': nz}, {'points': pts})
    pts = _points(17)
    bad = {'dtype': _points(17, dtype=torch.float64), 'dim': torch.zeros((17, 2, 3)), 'contiguity': _points(17, 12)[:, :6]}
    for name, fn in (('mean_vfe', ops.mean_vfe), ('mean_vfe_dev', ops.mean_vfe_dev)):
        for what, p in bad.items():
            rows['%s refusal: points %s' % (name, what)] = _run(rec, fn, (p, grid, 5), {'nz': nz}, {'points': p})
        for C in (ops.MEAN_VFE_MIN_FEATURES - 1, ops.MEAN_VFE_MAX_FEATURES + 1):
            rows['%s refusal: %d features' % (name, C)] = _run(rec, fn, (pts, grid, C), {'nz': nz}, {'points': pts})
        rows['%s refusal: row stride' % name] = _run(rec, fn, (pts, grid, 6), {'nz': nz}, {'points': pts})
        for B in (0, ops.MEAN_VFE_MAX_BATCH + 1):
            rows['%s refusal: batch %d' % (name, B)] = _run(rec, fn, (pts, ops.make_grid(VFE_RANGE, VFE_VOXEL, VFE_GRID, B), 5), {'nz': nz},
                                                            {'points': pts})
        for z in (0, ops.MEAN_VFE_MAX_NZ + 1):
            rows['%s refusal: nz %d' % (name, z)] = _run(rec, fn, (pts, grid, 5), {'nz': z}, {'points': pts})
        # the order of the checks: the first of several faults speaks
        rows['%s refusal: features before stride before batch before nz' % name] = _run(
            rec, fn, (pts, ops.make_grid(VFE_RANGE, VFE_VOXEL, VFE_GRID, 0), 6), {'nz': 0}, {'points': pts})
        rows['%s refusal: workspace size 0' % name] = _run(rec, fn, (pts, grid, 5), {'nz': nz}, {'points': pts},
                                                           script={'pcp_mean_vfe_workspace_bytes': 0})
        rows['%s scripted error word' % name] = _run(rec, fn, (pts, grid, 5), {'nz': nz}, {'points': pts}, script={'pcp_mean_vfe': (9, 3)})


def _table_rows(rec, ops, rows):
    B, sp = SHAPE4[0], SHAPE4[1:]
    for n in COUNTS:
        c, nd = _coords(n), _i32([n])
        for chk in (True, False):
            rows['spconv_table n=%d check_input=%s' % (n, chk)] = _run(rec, ops.spconv_table, (c, B, sp), {'check_input': chk}, {'coords': c})
        _twice(rec, rows, 'spconv_table_dev n=%d' % n, ops.spconv_table_dev, (c, nd, B, sp), {}, {'coords': c, 'n_dev': nd})
    c, nd = _coords(17), _i32([17])
    for chk in (True, False):                             # check_input False must not read, whatever the counters say
        rows['spconv_table distinct != n, check_input=%s' % chk] = _run(rec, ops.spconv_table, (c, B, sp), {'check_input': chk}, {'coords': c},
                                                                        script={'pcp_spconv_table_build': (15, 0)})
        rows['spconv_table bad flag, check_input=%s' % chk] = _run(rec, ops.spconv_table, (c, B, sp), {'check_input': chk}, {'coords': c},
                                                                   script={'pcp_spconv_table_build': (17, 1)})
        rows['spconv_table distinct != n and bad flag, check_input=%s' % chk] = _run(rec, ops.spconv_table, (c, B, sp), {'check_input': chk},
                                                                                     {'coords': c}, script={'pcp_spconv_table_build': (16, 1)})
    bad = {'dtype': torch.zeros((17, 4), dtype=torch.int64), 'columns': torch.zeros((17, 3), dtype=torch.int32),
           'dim': torch.zeros((17,), dtype=torch.int32), 'contiguity': torch.zeros((17, 8), dtype=torch.int32)[:, :4]}
    for what, t in bad.items():
        rows['spconv_table refusal: coords %s' % what] = _run(rec, ops.spconv_table, (t, B, sp), {}, {'coords': t})
        rows['spconv_table_dev refusal: coords %s' % what] = _run(rec, ops.spconv_table_dev, (t, nd, B, sp), {}, {'coords': t, 'n_dev': nd})
    rows['spconv_table refusal: table size 0'] = _run(rec, ops.spconv_table, (c, B, sp), {}, {'coords': c}, script={'pcp_spconv_table_bytes': 0})
    rows['spconv_table_dev refusal: table size 0'] = _run(rec, ops.spconv_table_dev, (c, nd, B, sp), {}, {'coords': c, 'n_dev': nd},
                                                          script={'pcp_spconv_table_bytes': 0})


def _subm_rows(rec, ops, rows):
    for n in COUNTS:
        c, nd = _coords(n), _i32([n])
        for perm in (True, False):
            t = _host_table(ops, n, perm=perm)
            named = dict(_named_table(t), coords=c, n_dev=nd)
            rows['spconv_build_subm n=%d perm=%s' % (n, perm)] = _run(rec, ops.spconv_build_subm, (c, t), {}, named)
            t.capacity = n
            rows['spconv_build_subm_dev n=%d perm=%s default name' % (n, perm)] = _run(rec, ops.spconv_build_subm_dev, (c, t, nd), {}, named)
        _twice(rec, rows, 'spconv_build_subm_dev n=%d' % n, ops.spconv_build_subm_dev, (c, t, nd), {'name': 'subm3'}, named)


def _strided_rows(rec, ops, rows):
    for geom, (k, s, p) in GEOMS.items():
        for n in COUNTS:
            c, nd, status = _coords(n), _i32([n]), torch.zeros((ops.DEV_STATUS_WORDS,), dtype=torch.int32)
            t = _host_table(ops, n)
            named = dict(_named_table(t), coords=c, n_dev=nd, status=status)
            rows['spconv_build_strided %s n=%d' % (geom, n)] = _run(rec, ops.spconv_build_strided, (c, t, k, s, p), {}, named)
            t.capacity = n
            osp = ops.spconv_out_shape(SHAPE4[1:], k, s, p)
            bound = ops.spconv_strided_bound(n, k, s, (SHAPE4[0],) + osp)
            for what, cap in (('None', None), ('below', max(bound - 1, 0)), ('above', bound + 5)):
                for st in (None, status):
                    rows['spconv_build_strided_dev %s n=%d capacity %s status %s' % (geom, n, what, 'given' if st is not None else 'None')] = _run(
                        rec, ops.spconv_build_strided_dev, (c, t, nd, k, s, p), {'capacity': cap, 'status': st, 'level': 2}, named)
            rows['spconv_build_strided_dev %s n=%d defaults' % (geom, n)] = _run(rec, ops.spconv_build_strided_dev, (c, t, nd, k, s, p), {}, named)
            _twice(rec, rows, 'spconv_build_strided_dev %s n=%d' % (geom, n), ops.spconv_build_strided_dev, (c, t, nd, k, s, p),
                   {'status': status, 'level': 1, 'name': 'strided1'}, named)
    c, nd, t = _coords(17), _i32([17]), _host_table(ops, 17)
    named = dict(_named_table(t), coords=c, n_dev=nd)
    rows['spconv_build_strided int arguments'] = _run(rec, ops.spconv_build_strided, (c, t, 3, 2, 1), {}, named)
    rows['spconv_build_strided_dev int arguments'] = _run(rec, ops.spconv_build_strided_dev, (c, t, nd, 3, 2, 1), {}, named)
    tiny = _host_table(ops, 17, shape4=(2, 1, 2, 2))
    refusals = {'kernel 4': ((3, 4, 3), 1, 0), 'kernel 0': ((0, 3, 3), 1, 0), 'stride 0': (3, (1, 0, 1), 1), 'stride 4': (3, 4, 1),
                'padding 3': (3, 1, (0, 0, 3)), 'padding -1': (3, 1, -1), 'kernel before stride before padding': (4, 4, 3)}
    for name, fn, extra in (('spconv_build_strided', ops.spconv_build_strided, ()), ('spconv_build_strided_dev', ops.spconv_build_strided_dev, (nd,))):
        for what, (k, s, p) in refusals.items():
            rows['%s refusal: %s' % (name, what)] = _run(rec, fn, (c, t) + extra + (k, s, p), {}, named)
        rows['%s refusal: no output left' % name] = _run(rec, fn, (c, tiny) + extra + (3, 1, 0), {}, dict(_named_table(tiny), coords=c, n_dev=nd))
        rows['%s refusal: table size 0' % name] = _run(rec, fn, (c, t) + extra + GEOMS['s2'], {}, named, script={'pcp_spconv_table_bytes': 0})


def _conv_rows(rec, ops, rows):
    def case(n_in, cin, cout, K=27, n_out=None, res=False, relu=False, ld=None, cin_pad=None, nbr=None, w=None, feats=None, residual=None):
        n_out = n_in if n_out is None else n_out
        if feats is None:
            feats = torch.zeros((n_in, ld or cin))[:, :cin] if ld else torch.zeros((n_in, cin))
        nbr = torch.zeros((K, n_out), dtype=torch.int32) if nbr is None else nbr
        w = torch.zeros((K, cout, cin_pad or (16 if cin <= 16 else cin))) if w is None else w
        bias = torch.zeros((cout,))
        if residual is None and res:
            residual = torch.zeros((n_out, cout))
        nd = _i32([n_out])
        named = {'features': feats, 'nbr': nbr, 'w_packed': w, 'bias': bias, 'residual': residual, 'n_dev': nd}
        return ((feats, nbr, w, bias), (feats, nbr, nd, w, bias)), {'residual': residual, 'relu': relu}, named

    def both(key, *a, **kw):
        (ha, da), k, named = case(*a, **kw)
        rows['spconv3d ' + key] = _run(rec, ops.spconv3d, ha, k, named)
        rows['spconv3d_dev ' + key] = _run(rec, ops.spconv3d_dev, da, k, named)
        return da, k, named
    for n in COUNTS:
        both('16 -> 16 n=%d' % n, n, 16, 16)
        both('32 -> 64 n=%d residual relu, 3 offsets, rows out != rows in' % n, n, 32, 64, K=3, n_out=(n + 1) // 2, res=True, relu=True)
    for cin, cout in ops.SPCONV_CHANNEL_PAIRS:
        for res, relu in ((False, False), (True, True)):
            both('%d -> %d res=%s relu=%s' % (cin, cout, res, relu), 17, cin, cout, res=res, relu=relu)
    both('cin 4 padded to 16', 17, 4, 16)
    both('cin 4 padded to 16, residual only', 17, 4, 16, res=True)
    both('cin 4 padded to 16, relu only', 17, 4, 16, relu=True)
    both('a features view with stride(0) != shape[1]', 17, 16, 32, ld=40)
    both('a one-row features view', 1, 16, 32, ld=40)
    da, k, named = both('default name', 17, 32, 32)
    _twice(rec, rows, 'spconv3d_dev 32 -> 32', ops.spconv3d_dev, da, dict(k, name='conv7'), named)
    both('refusal: channel pair 16 -> 48', 17, 16, 48)
    both('refusal: cin 2', 17, 2, 16)
    both('refusal: cin 24 padded to 32', 17, 24, 32, cin_pad=32)
    both('refusal: float16 features', 17, 16, 16, feats=torch.zeros((17, 16), dtype=torch.float16))
    both('refusal: float64 residual', 17, 16, 16, residual=torch.zeros((17, 16), dtype=torch.float64))
    both('refusal: int64 nbr', 17, 16, 16, nbr=torch.zeros((27, 17), dtype=torch.int64))
    both('refusal: nbr of one dimension', 17, 16, 16, nbr=torch.zeros((27,), dtype=torch.int32))
    both('refusal: int64 nbr before the channel pair', 17, 16, 48, nbr=torch.zeros((27, 17), dtype=torch.int64))
    both('refusal: nbr not contiguous', 17, 16, 16, nbr=torch.zeros((27, 34), dtype=torch.int32)[:, ::2])
    both('refusal: features of three dimensions', 17, 16, 16, feats=torch.zeros((17, 16, 1)))
    both('refusal: features columns strided', 17, 16, 16, feats=torch.zeros((17, 32))[:, ::2])
    both('refusal: weights of another K', 17, 16, 16, w=torch.zeros((9, 16, 16)))
    both('refusal: residual of another shape', 17, 16, 16, residual=torch.zeros((16, 16)))


def _dense_rows(rec, ops, rows):
    for n in COUNTS:
        f = torch.zeros((n, 32))
        t = _host_table(ops, n)
        named = dict(_named_table(t), features=f)
        rows['spconv_dense n=%d on a host table' % n] = _run(rec, ops.spconv_dense, (f, t), {}, named)
        t.capacity = n
        rows['spconv_dense n=%d on a table with a capacity' % n] = _run(rec, ops.spconv_dense, (f, t), {}, named)
    f = torch.zeros((17, 32))
    t = _host_table(ops, 17, perm=False)
    rows['spconv_dense on a table without a perm'] = _run(rec, ops.spconv_dense, (f, t), {}, dict(_named_table(t), features=f))
    t.capacity = 16
    rows['spconv_dense refusal: rows != capacity'] = _run(rec, ops.spconv_dense, (f, t), {}, dict(_named_table(t), features=f))
    deep = _host_table(ops, 17, shape4=(1, ops.MEAN_VFE_MAX_NZ + 1, 2, 2))
    rows['spconv_dense refusal: nz'] = _run(rec, ops.spconv_dense, (f, deep), {}, dict(_named_table(deep), features=f))
    h = torch.zeros((17, 32), dtype=torch.float16)
    rows['spconv_dense refusal: float16'] = _run(rec, ops.spconv_dense, (h, t), {}, dict(_named_table(t), features=h))


def _pure_rows(rec, ops, rows):
    levels = [('voxels', 100), ('spconv2', 50), ('spconv3', 25)]
    W = ops.DEV_STATUS_WORDS
    for err in (0, 1, 2, 3):
        for over in (0, 1, 2, 4, 5, 8, 6 | 1 << 30):
            words = [7, err, 7, 0] + [over] + [0] * (W - 5)
            for lv in (None, levels):
                rows['dev_status_check err %d overflow %d levels %s' % (err, over, 'given' if lv else 'None')] = _run(
                    rec, ops.dev_status_check, (words, 2, lv))
    rows['dev_status_check on a tensor of words'] = _run(rec, ops.dev_status_check, (_i32([0, 0, 0, 0, 2, 0, 0, 0]), 3, levels))
    for geom, (k, s, p) in GEOMS.items():
        out4 = (SHAPE4[0],) + ops.spconv_out_shape(SHAPE4[1:], k, s, p)
        sites = out4[0] * out4[1] * out4[2] * out4[3]
        for cap in (0, 1, 17, sites + 1):
            rows['spconv_strided_bound %s capacity %d' % (geom, cap)] = _run(rec, ops.spconv_strided_bound, (cap, k, s, out4))
        rows['spconv_out_shape %s' % geom] = _run(rec, ops.spconv_out_shape, (SHAPE4[1:], k, s, p))


def _layer_rows(rec, ops, rows):
    """SubM + BN + ReLU, a strided SparseConv3d with an indice_key, a SubM, and a second SubM that reuses the cached neighbour table"""
    from pcp_amd import spconv
    torch.manual_seed(0)
    net = spconv.SparseSequential(spconv.SubMConv3d(4, 16, 3, padding=1, bias=False, indice_key='subm1'), nn.BatchNorm1d(16), nn.ReLU(),
                                  spconv.SparseConv3d(16, 32, 3, stride=2, padding=1, bias=False, indice_key='spconv2'), nn.BatchNorm1d(32), nn.ReLU(),
                                  spconv.SubMConv3d(32, 32, 3, padding=1, indice_key='subm2'),
                                  spconv.SubMConv3d(32, 32, 3, padding=1, indice_key='subm2')).eval()

    def forward(x):
        with torch.no_grad():
            return net(x)

    def after(out):
        d = out.dev
        return {'out': {'features': rec.tensor(out.features), 'indices': rec.tensor(out.indices), 'spatial_shape': list(out.spatial_shape),
                        'capacity': out.capacity, 'n_dev': rec.value(out.n_dev), 'trusted_indices': out.trusted_indices,
                        'indice_dict': sorted(str(key if not isinstance(key, tuple) else key[0]) for key in out.indice_dict)},
                'dev': None if d is None else {'level': d.level, 'convs': d.convs, 'levels': [list(v) for v in d.levels]}}
    for n in COUNTS:
        f, c = torch.zeros((n, 4)), _coords(n)
        for trusted in (False, True):
            x = spconv.SparseConvTensor(f, c, SHAPE4[1:], SHAPE4[0])
            x.trusted_indices = trusted
            rows['layers n=%d host counts trusted_indices=%s' % (n, trusted)] = _run(rec, forward, (x,), {}, {'features': f, 'indices': c}, after=after)
        x = spconv.SparseConvTensor(f, c.long(), SHAPE4[1:], SHAPE4[0])
        rows['layers n=%d host counts, int64 indices' % n] = _run(rec, forward, (x,), {}, {'features': f}, after=after)
        for cap_name, row_capacity in (('None', None), ('given', [None, 5, None])):
            bufs = ops.DevBuffers()
            for i in (1, 2):
                nd, status = _i32([n]), torch.zeros((ops.DEV_STATUS_WORDS,), dtype=torch.int32)
                dev = spconv.DeviceCounts(status, bufs, row_capacity, input_capacity=n)
                x = spconv.SparseConvTensor(f, c, SHAPE4[1:], SHAPE4[0]).with_device_count(nd, dev)
                rows['layers n=%d device counts row_capacity %s forward %d' % (n, cap_name, i)] = _run_with_bufs(
                    rec, lambda: forward(x), {'features': f, 'indices': c, 'n_dev': nd, 'status': status}, bufs, after)


def _run_with_bufs(rec, fn, named, bufs, after):
    """as _run for a callable that reaches its DevBuffers by itself (the layers take them from the tensor)"""
    rec.begin(named, bufs, {})
    row = {}
    with _fakes(rec):
        try:
            row.update(after(fn()))
        except Exception as e:
            row['raises'] = [type(e).__name__, str(e)]
    row['calls'], row['reads'], row['bufs'] = rec.calls, rec.reads, rec.bufs_state()
    return row


def record():
    from pcp_amd import ops
    rec, rows = Recorder(), {}
    for part in (_mean_vfe_rows, _table_rows, _subm_rows, _strided_rows, _conv_rows, _dense_rows, _pure_rows, _layer_rows):
        part(rec, ops, rows)
    return json.loads(json.dumps(rows))                   # tuples as lists, as the file holds them


def main():
    head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip()
    with open(TABLE, 'w') as f:
        json.dump({'recorded_at': head, 'rows': record()}, f, indent=0, sort_keys=True)
        f.write('\n')
    print('wrote', TABLE)


if __name__ == '__main__':
    main()
