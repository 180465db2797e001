"""CPU: the step bookkeeping has one scalar rule (``TrainEngine._advance``, behind every step however it ran) and one
statement of it for k steps ahead (``replay_counters``, what ``program()`` writes into a replay table).  The two must
agree row by row, or a replay silently diverges from the eager step.  ``_advance`` reads and writes plain attributes
only, so it runs here on a stand-in that carries exactly those."""
import types

import pytest

from cmlpl_amd.engine import TrainEngine, replay_counters

BANK_STEP = 256
Q = 3 * BANK_STEP + 7          # small and odd: the pointers wrap three times inside K steps
K = 9
STARTS = [([0, 0], 0, 0), ([0, 256], 1, 1), ([519, 3], 5, 7), ([Q - 1, Q - 256], 40, 41), ([256, 0], 0, 12)]


def _state(ptr, adam_t, step_count, hist_rows, method):
    return types.SimpleNamespace(ptr=list(ptr), adam_t=adam_t, step_count=step_count, hist_rows=hist_rows, method=method,
                                 Q=Q, hp=types.SimpleNamespace(bank_step=BANK_STEP), _cur_row=0, _last_n=0)


@pytest.mark.parametrize("hist_rows", [1, 4])
@pytest.mark.parametrize("method", ["cmlpl", "cps"])
@pytest.mark.parametrize("ptr,adam_t,step_count", STARTS)
def test_rows_of_k_steps_ahead_are_the_states_of_k_scalar_advances(ptr, adam_t, step_count, hist_rows, method):
    rows = replay_counters(ptr, adam_t, step_count, Q, BANK_STEP, hist_rows, method, K + 1)     # row K: the state after K
    assert sorted(rows) == ["adam_t", "hist_row", "ptr", "step"]
    eng = _state(ptr, adam_t, step_count, hist_rows, method)
    for j in range(K + 1):
        # row j = the state BEFORE the (j+1)-th advance; its adam_t is that step's own (1-based), its hist_row the one
        # the advance records as written
        assert rows["ptr"][j].tolist() == eng.ptr, (j, rows["ptr"][j], eng.ptr)
        assert int(rows["step"][j]) == eng.step_count and int(rows["adam_t"][j]) == eng.adam_t + 1
        if j == K:
            break
        TrainEngine._advance(eng, 24)
        assert int(rows["hist_row"][j]) == eng._cur_row == (eng.step_count - 1) % hist_rows
        assert eng._last_n == 24
    assert eng.step_count == step_count + K and eng.adam_t == adam_t + K
    if method == "cps":        # no memory bank: the pointers never move
        assert eng.ptr == list(ptr) and (rows["ptr"] == ptr).all()
    else:                      # train.py:234,237: ptr0 by the literal step, ptr1 follows ptr0 -- from the first advance on
        assert eng.ptr == [(ptr[0] + K * BANK_STEP) % Q, (ptr[0] + (K + 1) * BANK_STEP) % Q]
        assert rows["ptr"][0].tolist() == list(ptr)
        assert len({int(p) for p in rows["ptr"][:, 0]}) == K + 1 and (rows["ptr"][:, 0] < BANK_STEP).sum() >= 3   # wrapped


def test_a_step_without_update_advances_the_step_counter_and_leaves_adam_t():
    eng = _state([519, 3], 5, 7, 4, "cmlpl")
    TrainEngine._advance(eng, 8, apply_update=False)
    assert (eng.step_count, eng.adam_t, eng._cur_row, eng._last_n) == (8, 5, 3, 8)
    assert eng.ptr == [(519 + BANK_STEP) % Q, (519 + 2 * BANK_STEP) % Q]
    TrainEngine._advance(eng, 8, apply_update=True, row=0)       # (a caller that has formed the ring row hands it in)
    assert (eng.step_count, eng.adam_t, eng._cur_row) == (9, 6, 0)
