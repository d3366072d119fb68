"""CPU: what the bf16-pipe sparse convolutions (csrc/spconv_os_x3.hip, csrc/spconv_os_x6.hip, csrc/spconv_os_bf16.hip - the three
policies of csrc/spconv_os_mma.h) decide on the host, against a table recorded from the library before the three files were
folded into one template (tools/make_spconv_plan_golden.py -> tests/golden/spconv_os_plan.json): return code and outputs of
sst_spconv_conv_os_plan for the entries F32X3, F32X6, ROWS_F32X6 and ROWS_BF16, and the three workspace-size queries, over row
counts, offsets, channel shapes and workspace sizes that reach both column classes, every split factor, the split halved for
lack of room and each refusal.  No kernel is launched."""
import json
import os

import pytest

from tools import make_spconv_plan_golden as G


@pytest.fixture(scope='module')
def tables():
    overrides = [v for v in G.SPLIT_OVERRIDES if v in os.environ]
    if overrides:
        pytest.skip('%s is set: the library caches the split override at first use, the table holds its own choice'
                    % ', '.join(overrides))
    from sst_amd import _lib
    with open(G.GOLDEN) as f:
        return G.collect(_lib.load()), json.load(f)


def test_the_table_covers_every_branch_of_the_pick(tables):
    _, want = tables
    assert [want[k] for k in ('m', 'kvol', 'channels', 'workspaces')] == [
        list(G.M), list(G.KVOL), [list(c) for c in G.CHANNELS], list(G.WORKSPACES)]
    for entry in ('ROWS_F32X6', 'ROWS_BF16'):
        ok = [r for r in want['plan'][entry] if r[0] == 0]
        assert {r[2] for r in ok} == {64, 128} and {r[3] for r in ok} == {1, 2, 4, 8}
        assert {r[0] for r in want['plan'][entry]} == {0, -1, -2}           # SST_OK, SST_ERR_ARG, SST_ERR_UNSUPPORTED
    assert {r[3] for r in want['plan']['F32X3'] if r[0] == 0} == {1}
    assert all(r[1:] == [G.UNTOUCHED] * 4 for e in G.ENTRIES for r in want['plan'][e] if r[0] != 0)


@pytest.mark.parametrize('entry', list(G.ENTRIES))
def test_launch_plans_are_those_of_the_table(tables, entry):
    got, want = tables
    assert len(got['plan'][entry]) == len(want['plan'][entry]) >= 432
    assert got['plan'][entry] == want['plan'][entry]


@pytest.mark.parametrize('query', ['f32x6_workspace_bytes', 'f32x6_workspace_bytes_rows', 'bf16_workspace_bytes_rows'])
def test_workspace_sizes_are_those_of_the_table(tables, query):
    got, want = tables
    assert len(want[query]) >= 54 and got[query] == want[query]
