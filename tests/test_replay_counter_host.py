"""The accounting of graphstep.ReplayCounter in numbers, without a GPU: a plain PhiloxStream and a CPU int64 tensor as the device word.

A replay is simulated by what it does to the word -- the staging launch's bump entry in front of the graph (``staged``), or the
graph's own advance behind its kernels (the two-graph step) -- and an eager fallback by entering ReplayCounter.eager, taking blocks
from the stream and leaving.  The kernels of a step add the word to offsets that count from ``base``, so a step that finds the word at
c and draws d blocks uses [base + c, base + c + d)."""
import pytest
import torch

from fragnet_amd.graphstep import ReplayCounter
from fragnet_amd.ops import PhiloxStream

WARM = 3        # warm-up steps in front of the capture


def captured(per_step, staged, seed, what="Philox"):
    """A counter after warm-up and capture of a step that draws ``per_step`` blocks, and its bump entry (None: nothing is staged)."""
    stream = PhiloxStream(seed=seed)
    c = ReplayCounter(stream, torch.zeros(1, dtype=torch.int64), what)
    assert stream.dev is c.word
    for _ in range(WARM):
        c.mark()
        stream.take(4 * per_step)
        c.measure()
    c.mark()
    stream.take(4 * per_step)           # the captured step: these offsets are baked in
    c.check()
    assert (c.base, c.per_step, c.drawn()) == (WARM * per_step, per_step, per_step)
    entry = c.stage() if staged else None
    assert c.staged == staged and int(c.word) == (-per_step if staged else 0)
    return c, entry


def replay(c, entry):
    """-> the word as the replayed kernels see it"""
    if c.staged:
        if entry is not None:
            word, inc = entry
            assert word is c.word and inc == c.per_step
            word += inc
        return int(c.word)
    seen = int(c.word)
    c.stream.dev += c.per_step          # what rng.advance_device(consumed), captured behind the kernels, does on every replay
    return seen


def eager(counters, blocks):
    """one fallback step over all ``counters``; counter i draws blocks[i] -> [(word as the eager kernels see it, blocks drawn)]"""
    before = [c.stream.offset for c in counters]
    with ReplayCounter.eager(*counters):
        seen = [int(c.word) for c in counters]
        for c, n in zip(counters, blocks):
            assert c.stream.offset == c.base            # it draws from where the captured step's offsets start
            if n:
                c.stream.take(4 * n - 1)                  # take() counts numbers, four to a block, rounded up
        drawn = [c.drawn() for c in counters]
    assert [c.stream.offset for c in counters] == before  # the host offsets are what they were
    return list(zip(seen, drawn))


def sequence(counters, entries, big):
    """replay, replay, an eager step that draws big[i] > per_step, replay, replay -> per counter the five block ranges"""
    ranges = [[] for _ in counters]

    def note(i, c, seen, drawn):
        ranges[i].append((c.base + seen, c.base + seen + drawn))
    for step in range(5):
        if step == 2:
            for i, (c, (seen, drawn)) in enumerate(zip(counters, eager(counters, big))):
                assert drawn == big[i] > c.per_step
                note(i, c, seen, drawn)
        else:
            for i, (c, e) in enumerate(zip(counters, entries)):
                note(i, c, replay(c, e), c.per_step)
    return ranges


@pytest.mark.parametrize("staged", [True, False])
def test_replays_and_an_eager_step_never_share_a_block(staged):
    per_step, big = 10, 17
    c, entry = captured(per_step, staged, seed=1)
    host = c.stream.offset
    (ranges,) = sequence([c], [entry], [big])
    b = c.base
    assert ranges == [(b, b + 10), (b + 10, b + 20), (b + 20, b + 37), (b + 37, b + 47), (b + 47, b + 57)]
    assert ranges[0][0] == c.base and ranges == sorted(ranges)
    for (lo, hi), (lo2, hi2) in zip(ranges, ranges[1:]):
        assert lo < hi <= lo2 < hi2                       # ascending and pairwise disjoint
    assert c.stream.offset == host
    # between replays the word is one step behind exactly when the staging launch moves it
    assert int(c.word) == (57 - per_step if staged else 57)


@pytest.mark.parametrize("staged", [True, False])
def test_an_eager_step_that_draws_what_a_replay_draws_moves_the_word_like_one(staged):
    a, entry_a = captured(10, staged, seed=1)
    b, entry_b = captured(10, staged, seed=1)
    for c, e in ((a, entry_a), (b, entry_b)):
        replay(c, e)
    seen_a = replay(a, entry_a)
    ((seen_b, drawn),) = eager([b], [10])
    assert (seen_b, drawn) == (seen_a, 10) and int(b.word) == int(a.word)
    assert replay(a, entry_a) == replay(b, entry_b) == 20


@pytest.mark.parametrize("staged", [True, False])
def test_an_eager_step_that_draws_nothing(staged):
    # a model without dropout: nothing per step, no bump entry, and the word stays where replays leave it -- at 0
    c, entry = captured(0, staged, seed=1)
    assert entry is None
    assert replay(c, entry) == 0
    assert eager([c], [0]) == [(0, 0)] and int(c.word) == 0
    assert replay(c, entry) == 0
    # a step that draws per replay but nothing in this eager pass (evaluation-mode layers, say) consumes no block: the word is back where
    # the step found it, and the next replay uses the range this one would have
    c, entry = captured(10, staged, seed=1)
    assert replay(c, entry) == 0
    word = int(c.word)
    ((seen, drawn),) = eager([c], [0])
    assert (seen, drawn) == (10, 0) and int(c.word) == word
    assert replay(c, entry) == 10


def test_two_counters_keep_to_their_own_words():
    """dropout and mask streams through the same steps: each word goes where it goes when its counter is driven alone"""
    alone = []
    for per_step, big, seed, what in ((10, 17, 1, "Philox"), (3, 8, 2, "mask")):
        c, entry = captured(per_step, True, seed, what)
        alone.append((sequence([c], [entry], [big])[0], int(c.word)))
    drop, e_drop = captured(10, True, 1)
    mask, e_mask = captured(3, True, 2, "mask")
    assert drop.word is not mask.word and drop.stream is not mask.stream
    both = sequence([drop, mask], [e_drop, e_mask], [17, 8])
    assert [(both[0], int(drop.word)), (both[1], int(mask.word))] == alone
    assert int(drop.word) == 57 - 10 and int(mask.word) == (3 + 3 + 8 + 3 + 3) - 3


def test_a_captured_step_that_draws_differently_is_refused():
    for what in ("Philox", "mask"):
        stream = PhiloxStream(seed=1)
        c = ReplayCounter(stream, torch.zeros(1, dtype=torch.int64), what)
        c.mark()
        stream.take(40)
        c.measure()
        c.mark()
        stream.take(44)
        with pytest.raises(RuntimeError, match=f"the captured step drew a different number of {what} blocks than the warm-up steps"):
            c.check()
