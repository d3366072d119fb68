#!/usr/bin/env python
"""Host-only record of what the bf16-pipe sparse convolutions (csrc/spconv_os_x3.hip, _x6.hip, _bf16.hip: the policies of
csrc/spconv_os_mma.h) decide before they launch: for every entry of sst_spconv_conv_os_plan but the fp32 one the return code and
the four outputs, and the three workspace-size queries, over a grid that reaches both column classes, every split factor 1 .. 8,
the split halved for lack of room and each refusal.  No kernel is launched, no GPU is needed.

    python tools/make_spconv_plan_golden.py            # writes tests/golden/spconv_os_plan.json

tests/test_spconv_plan_host.py asserts that the library still answers what the table holds.  The split override variables
(SST_SPCONV_X6_SPLIT, SST_SPCONV_BF16_SPLIT) must be unset: the library reads them once."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'spconv_os_plan.json')

M = (1, 64, 65, 258, 1866, 6542, 131072, 262144)
KVOL = (1, 3, 8, 27, 32, 33)
CHANNELS = ((4, 4), (12, 20), (16, 7), (64, 64), (64, 66), (68, 132), (128, 160), (256, 256), (5, 7))
WORKSPACES = ('packed', 'rows', 'packed-1', 'midway', 'none')
ENTRIES = {'F32X3': 1, 'F32X6': 2, 'ROWS_F32X6': 3, 'ROWS_BF16': 4}     # SST_SPCONV_OS_ENTRY_*
UNTOUCHED = -7                                                          # what the outputs hold before the call
SPLIT_OVERRIDES = ('SST_SPCONV_X6_SPLIT', 'SST_SPCONV_BF16_SPLIT')


def workspace(lib, entry, which, m, kvol, cin, cout):
    """the workspace size a plan query is told: the packed weights alone, what the _rows query asks for, one byte less than the
    packed weights, halfway between the first two (room for some of the partial tiles: the split is halved), nothing"""
    if entry == 'ROWS_BF16':
        packed = lib.sst_spconv_conv_os_bf16_workspace_bytes_rows(kvol, cin, cout, 0)
        rows = lib.sst_spconv_conv_os_bf16_workspace_bytes_rows(kvol, cin, cout, m)
    else:
        packed = lib.sst_spconv_conv_os_f32x6_workspace_bytes(kvol, cin, cout)
        rows = lib.sst_spconv_conv_os_f32x6_workspace_bytes_rows(kvol, cin, cout, m)
    return {'packed': packed, 'rows': rows, 'packed-1': packed - 1, 'midway': (packed + rows) // 2, 'none': 0}[which]


def plan(lib, entry, m, kvol, cin, cout, workspace_bytes):
    """[return code, tile rows, columns, split, workgroups]"""
    tr, cols, ns = (ctypes.c_int32(UNTOUCHED) for _ in range(3))
    wgs = ctypes.c_int64(UNTOUCHED)
    rc = lib.sst_spconv_conv_os_plan(ENTRIES[entry], m, kvol, cin, cout, 0, workspace_bytes, ctypes.byref(tr), ctypes.byref(cols),
                                     ctypes.byref(ns), ctypes.byref(wgs))
    return [rc, tr.value, cols.value, ns.value, wgs.value]


def collect(lib):
    """every record, in the nesting order m, kvol, channels(, workspace)"""
    shapes = [(m, kvol, cin, cout) for m in M for kvol in KVOL for cin, cout in CHANNELS]
    out = {'m': list(M), 'kvol': list(KVOL), 'channels': [list(c) for c in CHANNELS], 'workspaces': list(WORKSPACES),
           'untouched': UNTOUCHED, 'plan': {}}
    for entry in ENTRIES:
        told = WORKSPACES if entry.startswith('ROWS') else WORKSPACES[:1]     # the other two entries are not told a size
        out['plan'][entry] = [plan(lib, entry, m, kvol, cin, cout, workspace(lib, entry, w, m, kvol, cin, cout))
                              for m, kvol, cin, cout in shapes for w in told]
    out['f32x6_workspace_bytes'] = [lib.sst_spconv_conv_os_f32x6_workspace_bytes(kvol, cin, cout)
                                    for kvol in KVOL for cin, cout in CHANNELS]
    out['f32x6_workspace_bytes_rows'] = [lib.sst_spconv_conv_os_f32x6_workspace_bytes_rows(kvol, cin, cout, m)
                                         for m, kvol, cin, cout in shapes]
    out['bf16_workspace_bytes_rows'] = [lib.sst_spconv_conv_os_bf16_workspace_bytes_rows(kvol, cin, cout, m)
                                        for m, kvol, cin, cout in shapes]
    return out


def main():
    sys.path.insert(0, ROOT)
    from sst_amd import _lib
    if any(v in os.environ for v in SPLIT_OVERRIDES):
        sys.exit('unset %s first' % ' / '.join(SPLIT_OVERRIDES))
    with open(GOLDEN, 'w') as f:
        json.dump(collect(_lib.load()), f, separators=(',', ':'))
        f.write('\n')
    print('wrote', GOLDEN)


if __name__ == '__main__':
    main()
