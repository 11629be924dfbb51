"""Host bookkeeping of set_points' steady path (nufft_steady_path_observe: plan_engines.cpp steady_observe / steady_eligible), no device:
the host takes the steady path while the NEWEST feedback record it has seen reports a streak of at least three point sets that both rings served."""
import ctypes as C


def _observe(state, seq, streak):
    from nufft_pkg import nufft
    assert nufft.lib.nufft_steady_path_observe(state, seq, streak) == 0
    return state[1]


def test_streak_of_three_opens_the_steady_path_and_a_miss_closes_it():
    state = (C.c_uint32 * 2)(0, 0)
    assert _observe(state, 0, 0) == 0                      # plan creation: no record yet
    assert [_observe(state, seq, seq) for seq in (1, 2)] == [0, 0]
    assert _observe(state, 3, 3) == 1 and list(state) == [3, 1]
    assert _observe(state, 4, 4) == 1
    assert _observe(state, 5, 0) == 0 and list(state) == [5, 0]      # a set the rings would not have served: streak 0
    assert [_observe(state, seq, seq - 5) for seq in (6, 7, 8, 9)] == [0, 0, 1, 1]


def test_a_record_is_counted_once_and_may_be_many_calls_old():
    state = (C.c_uint32 * 2)(0, 0)
    # the host runs ahead: the first record it sees is that of the 20th point set
    assert _observe(state, 20, 17) == 1
    # the same record again (nothing new has arrived), whatever the other words read meanwhile: no change
    assert _observe(state, 20, 0) == 1 and list(state) == [20, 1]
    # records skipped in between do not matter: the streak is the device's own count
    assert _observe(state, 31, 2) == 0
    assert _observe(state, 31, 9) == 0
    assert _observe(state, 40, 11) == 1
    # sequence numbers wrap
    assert _observe(state, 0xFFFFFFFF, 5) == 1 and _observe(state, 0, 0) == 0


def test_null_state_is_refused():
    from nufft_pkg import nufft
    assert nufft.lib.nufft_steady_path_observe(None, 1, 3) == 1      # NUFFT_ERR_INVALID_ARG
