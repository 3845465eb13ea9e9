"""The host loop of the iterated passes (``ops._to_fixpoint``: launch a batch of rounds, read the batch's "changed" flags once, return
the round that changed nothing, raise after the limit) and its four callers ``split_regrow``, ``mask_flood``,
``skeleton_thin_level`` and ``pick_select``, without a device: the helper with a scripted ``launch``, the callers on host tensors
with ``ops.call`` replaced by a function that writes scripted flags where the library would."""

from __future__ import annotations

import ctypes

import pytest
import torch

from cryovit_amd import _lib
from cryovit_amd.engine import ops


class Rounds:
    """Rounds 1 .. fix - 1 change something, round ``fix`` and all after it nothing (fix = None: every round changes something)."""

    def __init__(self, fix):
        self.fix, self.done, self.batches = fix, 0, []

    def flags(self, n: int) -> list[int]:
        out = [int(self.fix is None or self.done + i + 1 < self.fix) for i in range(n)]
        self.done += n
        self.batches.append(n)
        return out


# batch, limit, the round that changes nothing -> the batches launched
CASES = [
    (4, 100, 1, [4]),  # the first slot of a batch
    (4, 100, 2, [4]),  # a middle slot
    (4, 100, 4, [4]),  # the last slot
    (4, 100, 5, [4, 4]),  # the first slot of the second batch
    (4, 100, 11, [4, 4, 4]),
    (4, 6, 5, [4, 2]),  # the last batch cut short by the limit, the fixpoint in it
    (4, 6, 6, [4, 2]),  # ... in its last slot
    (1, 3, 3, [1, 1, 1]),
    (5, 3, 2, [3]),  # a batch above the limit
]


@pytest.mark.parametrize("batch,limit,fix,batches", CASES)
def test_helper_returns_the_round_that_changed_nothing(batch, limit, fix, batches):
    r = Rounds(fix)
    assert ops._to_fixpoint(r.flags, batch, limit, "never") == fix
    assert r.batches == batches


@pytest.mark.parametrize("batch,limit,fix,batches", [(4, 6, 7, [4, 2]), (4, 8, None, [4, 4]), (4, 1, 2, [1]), (3, 7, None, [3, 3, 1])])
def test_helper_raises_after_the_limit(batch, limit, fix, batches):
    r = Rounds(fix)
    with pytest.raises(_lib.CvxError, match="^somebody: the text of the caller$"):
        ops._to_fixpoint(r.flags, batch, limit, "somebody: the text of the caller")
    assert r.batches == batches and r.done == limit  # never a round past the limit


# ---- the callers ----

ROUNDS_ARG = {"cvx_split_rounds": -2, "cvx_mask_flood_rounds": -2, "cvx_skeleton_cycles": -2, "cvx_pick_rounds": -5}  # changed is the last


@pytest.fixture
def host(monkeypatch):
    """ops on host tensors: the library is loaded but never called.  Returns a function that installs the script of a run and
    returns it; its ``calls`` lists (entry, arguments) of every call."""
    _lib.load()  # the callers look the entry up before they call

    def install(fix):
        r = Rounds(fix)
        r.calls = []

        def fake_call(dev, what, fn, *args):
            n = args[ROUNDS_ARG[what]]
            (ctypes.c_int32 * n).from_address(args[-1])[:] = r.flags(n)
            r.calls.append((what, args))

        monkeypatch.setattr(ops, "call", fake_call)
        return r

    monkeypatch.setattr(ops, "_dev_check", lambda *ts: torch.device("cpu"))
    return install


SHAPE = (2, 3, 70)


def run_split(max_rounds):
    return ops.split_regrow(torch.zeros(SHAPE, dtype=torch.int32), torch.zeros(SHAPE, dtype=torch.int64), max_rounds=max_rounds)


def run_flood(max_rounds):
    words = (SHAPE[0], SHAPE[1], 2)
    return ops.mask_flood(torch.zeros(words, dtype=torch.int64), torch.zeros(words, dtype=torch.int64), SHAPE, max_rounds=max_rounds)


def run_thin(max_rounds):
    return ops.skeleton_thin_level(torch.zeros(SHAPE, dtype=torch.int32), torch.ones(SHAPE, dtype=torch.int32), 1, 3, 4, max_cycles=max_rounds)


def run_pick(max_rounds):
    state = torch.zeros((2, SHAPE[0], SHAPE[1], 2), dtype=torch.int64)
    return ops.pick_select(torch.ones(SHAPE, dtype=torch.int32), 1, state, spacing=2, max_rounds=max_rounds)[1]


CALLERS = {
    "split_regrow": (run_split, "SPLIT_ROUND_BATCH", "split_regrow: no fixpoint after max_rounds = 6 rounds"),
    "mask_flood": (run_flood, "MASK_ROUND_BATCH", "mask_flood: no fixpoint after max_rounds = 6 rounds"),
    "skeleton_thin_level": (run_thin, "SKELETON_CYCLE_BATCH", "skeleton_thin_level: level 3 has no fixpoint after max_cycles = 6 cycles"),
    "pick_select": (run_pick, "PICK_ROUND_BATCH", "pick_select: no fixpoint after max_rounds = 6 rounds"),
}


@pytest.mark.parametrize("name", CALLERS)
def test_caller_counts_rounds_and_reads_its_batch_constant_at_call_time(name, host, monkeypatch):
    run, constant, _ = CALLERS[name]
    assert getattr(ops, constant) == 4
    r = host(6)
    assert run(6) == 6 and r.batches == [4, 2]
    r = host(2)
    assert run(4096) == 2 and r.batches == [4]
    monkeypatch.setattr(ops, constant, 3)
    r = host(7)
    assert run(4096) == 7 and r.batches == [3, 3, 3]


@pytest.mark.parametrize("name", CALLERS)
def test_caller_raises_in_its_own_words(name, host):
    run, _, text = CALLERS[name]
    r = host(7)
    with pytest.raises(_lib.CvxError) as e:
        run(6)
    assert str(e.value) == text and r.batches == [4, 2]


def test_pick_select_swaps_its_states_after_an_odd_batch(host, monkeypatch):
    labels = torch.ones(SHAPE, dtype=torch.int32)
    state = torch.zeros((2, SHAPE[0], SHAPE[1], 2), dtype=torch.int64)
    r = host(9)
    got, rounds = ops.pick_select(labels, 1, state, spacing=2, batch=3)
    a, b = state.data_ptr(), [args[9] for _, args in r.calls][0]
    # a round reads state_a and writes state_b: after 3 rounds the newest state is b, after 6 it is a again
    assert [(args[8], args[9]) for _, args in r.calls] == [(a, b), (b, a), (a, b)] and rounds == 9
    assert got.data_ptr() == a  # the batch with the fixpoint is not swapped: both states hold it
    r = host(9)
    got, rounds = ops.pick_select(labels, 1, state, spacing=2, batch=4)
    assert [args[8] for _, args in r.calls] == [a, a, a] and got.data_ptr() == a and rounds == 9
    r = host(5)
    got, rounds = ops.pick_select(labels, 1, state, spacing=2, batch=3)
    assert got.data_ptr() != a and rounds == 5  # three rounds ended in the other state, the fixpoint came in the batch after
