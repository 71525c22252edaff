"""Records tests/golden/workspace_bytes.json: the value of every workspace / table size query of the C library whose layout function
carves its fields on 256-byte boundaries, over a few dozen argument sets each (n = 0 and 1, sizes one below and one above a multiple of
256 bytes, both record strides of the rows pillariser).  The queries are plain host functions: no GPU is needed.
pcp_hunter_loss_workspace_bytes ends with the temporary storage hipCUB's radix sort asks for, which for tens of thousands of keys depends
on the device the host sees (1 823 232 bytes without one, 2 063 104 on an MI355X at n = 30 000); its rows stop at n = 1 000, where the sort
is one block and asks for none on either host, so the table holds only what this library's own layout decides.

The committed file was recorded with the library of the commit before csrc/pcp_common.h's PcpCarver replaced the seven written-out
carving lambdas (the file names that commit); tests/test_host_cpu.py replays it against the built library.

    PCP_HIP_LIB=<the library to record> python tests/golden/make_workspace_bytes.py <commit it was built from>
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, 'workspace_bytes.json')
sys.path.insert(0, os.path.join(HERE, '..', '..', 'practical-collab-perception_amd'))

# (nx, ny, batch): a 1-cell grid, cell counts around a multiple of 64 (256 bytes of int32), the mini fixture's grid, a full-size one
GRIDS = [(1, 1, 1), (7, 9, 1), (8, 8, 1), (5, 13, 1), (64, 64, 2), (432, 496, 1), (512, 512, 4)]
# rows: 0, 1, around 64 rows (256 bytes of int32), around 16 and 30 (the long-pillar and tile divisors), around a 1024-row tile, large
POINTS = [0, 1, 15, 16, 17, 29, 30, 31, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4097, 30000, 65536, 300001, 2000000]


def _grid_cases(extra=()):
    """every row count on two grids, every grid on three row counts"""
    seen, out = set(), []
    for g in ((7, 9, 1), (432, 496, 1)):
        for n in POINTS:
            seen.add((g, n))
    for g in GRIDS:
        for n in (0, 65, 30000):
            seen.add((g, n))
    for g, n in sorted(seen):
        for e in (extra or ((),)):
            out.append((g, n) + tuple(e))
    return out


def cases():
    """name -> list of argument tuples (a grid is its (nx, ny, batch) triple)"""
    c = {}
    c['pcp_voxelize_workspace_bytes'] = _grid_cases()
    c['pcp_pillarise_rows_workspace_bytes'] = _grid_cases(extra=((5,), (11,)))
    c['pcp_hard_voxelize_workspace_bytes'] = _grid_cases()
    c['pcp_mean_vfe_workspace_bytes'] = _grid_cases()
    c['pcp_spconv_table_bytes'] = [(b, d, h, w) for b in (1, 2, 4) for (d, h, w) in
                                   ((1, 1, 1), (1, 1, 63), (1, 1, 64), (1, 1, 65), (1, 8, 8), (3, 7, 13), (2, 32, 32), (2, 32, 33), (1, 64, 1023),
                                    (1, 64, 1024), (1, 64, 1025), (41, 160, 176), (5, 200, 176))]
    c['pcp_nms_workspace_bytes'] = [(n, b) for b in (1, 2, 4, 15, 16, 17) for n in (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 500, 4096)]
    c['pcp_bev_scatter_mean_workspace_bytes'] = [(b, h, w, n) for (b, h, w) in ((1, 1, 1), (1, 7, 9), (1, 8, 8), (2, 13, 5), (4, 128, 128))
                                                 for n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 30000, 300001)]
    c['pcp_hunter_loss_workspace_bytes'] = [(n, nf, nl, ch) for (n, nf) in ((0, 0), (1, 0), (1, 1), (21, 20), (22, 22), (63, 31), (64, 64), (65, 33),
                                                                           (1000, 255), (1000, 256), (1000, 257), (1000, 1000))
                                            for (nl, ch) in ((0, 1), (1, 32), (2, 32), (3, 32), (40, 64), (41, 96))]
    return c


def record():
    """name -> list of [arguments..., value] with the library pcp_amd.lib loads"""
    from pcp_amd import lib
    L = lib.load()
    out = {}
    for name, rows in cases().items():
        fn = getattr(L, name)
        got = []
        for args in rows:
            if isinstance(args[0], tuple):
                nx, ny, batch = args[0]
                g = lib.Grid(0.0, -40.0, -3.0, 0.16, 0.16, 4.0, nx, ny, batch)
                v = fn(ctypes.byref(g), *args[1:])
                got.append([nx, ny, batch] + list(args[1:]) + [int(v)])
            else:
                got.append(list(args) + [int(fn(*args))])
        out[name] = got
    return out


if __name__ == '__main__':
    doc = {'recorded_at': sys.argv[1] if len(sys.argv) > 1 else 'unknown', 'columns': 'arguments in the order of the C declaration (a grid as nx, ny, batch_size), then the value',
           'table': record()}
    with open(TABLE, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print({k: len(v) for k, v in doc['table'].items()})
