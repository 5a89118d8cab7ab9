"""Every launch path against every shipped kernel instance, bit for bit (tests/_launch_matrix.py: the invariant, the rows, the scripts, and
why a workgroup without a valid lane can neither hang nor write).  Sixteen rows by name on the diagnostics library, eight on the product
library through the scenes that reach them; seven scripts per row; every launch followed by the assertion that the row's instance rendered
it; every comparison of bits or exact integers against the row's own straight renders, which for a parity row are the oracle's.

That the module is not vacuous was tried on scratch copies of the sources (not kept): see profiles/HISTORY.md (r35)."""
import pytest

import _launch_matrix as M

pytestmark = pytest.mark.gpu


def _param(row, *more):
    return pytest.param(row, *more, id="-".join((M.row_id(row),) + more))


@pytest.mark.parametrize("row", [_param(r) for r in M.ROWS if not r.fast])
def test_a_parity_row_s_straight_renders_are_the_oracle_s(row):
    """The existing criterion, restated so that the module stands alone: 2, 3, 4, 6, 7 and 8 passes on the default stream, 3 and 7 on stream 3,
    each one launch on a fresh context -- colours, seeds, packed pixels and the five counters (M.reference compares before it hands out)."""
    for p, stream_id in ((2, 0), (3, 0), (4, 0), (6, 0), (7, 0), (8, 0), (3, M.STREAM), (7, M.STREAM)):
        assert M.reference(row, p, stream_id)["counters"] == M.oracle_frame(row.scene, p, stream_id)["counters"]
    assert not (M.bits(M.reference(row, 7)["colors"]) == M.bits(M.reference(row, 7, M.STREAM)["colors"])).all()     # another stream, another frame


@pytest.mark.parametrize("row", [_param(r) for r in M.ROWS if r.fast])
def test_a_fast_row_s_straight_render_is_a_function_of_its_inputs(row):
    """Fast mode has no bit-exact outside reference: the row's straight render is the only one.  The control: two fresh contexts render the
    same six passes to the same words.  A row that fails this is a finding about its instance (M.NOT_A_FUNCTION_OF_ITS_INPUTS names the cause
    and marks the row's scripts), not a reason to compare with a tolerance."""
    M.compare(M.straight(row, 6), M.reference(row, 6), what="%s rendered twice" % M.row_id(row))
    M.compare(M.straight(row, 7, M.STREAM), M.reference(row, 7, M.STREAM), what="%s rendered twice on stream %d" % (M.row_id(row), M.STREAM))
    assert not (M.bits(M.reference(row, 7)["colors"]) == M.bits(M.reference(row, 7, M.STREAM)["colors"])).all()


def _cell(row, script):
    cause = M.NOT_A_FUNCTION_OF_ITS_INPUTS.get(M.row_id(row))
    marks = [pytest.mark.xfail(strict=True, reason=cause)] if cause else []
    return pytest.param(row, script, id="%s-%s" % (M.row_id(row), script), marks=marks)


@pytest.mark.parametrize("row,script", [_cell(row, script) for row, script in M.CELLS])
def test_a_launch_path_leaves_the_words_of_the_straight_render(row, script):
    M.SCRIPTS[script](row)
