"""asl_set_window_pair_budget, the pair budget of the window-only searches, without a GPU: the
library exports it, a call returns the previous budget, and budgets that are not positive are
rejected with ASL_ERR_INVALID and leave the budget as it was."""


def test_window_pair_budget_setter():
    from ann_solo_amd import _lib
    L = _lib.lib()
    assert 'asl_set_window_pair_budget' in _lib.EXPORTS
    f = L.asl_set_window_pair_budget
    prev = f(1000)
    try:
        assert prev == 1 << 28                 # the default: 2 GiB of pair scores
        assert f(7) == 1000
        assert f(0) == -1                      # ASL_ERR_INVALID
        assert b'positive' in L.asl_last_error()
        assert f(-1) == -1
        assert f(1 << 40) == 7                 # the rejected calls changed nothing
        assert f(1) == 1 << 40
    finally:
        f(prev)
    assert f(prev) == prev
