"""The boundary planner's ALGORITHM (tp_boundaries_kernel, restated plainly in helpers/tp_planner_reference.py) against an
exhaustive optimum, on a seeded family of energy maps; no GPU.  tests/test_tp_planner_gpu.py holds the kernels to the
same reference, so what is shown here about the reference's plans holds for the device's.

Held on every map:
  * without forced cuts every cut is an allowed instant (quiet from 8 readings before it to one after it);
  * at most K pieces, the last one 2 readings at least, and without forced cuts every one (ref.check_cuts);
  * opt <= longest piece <= opt + 1 reading, opt from a dynamic programme over ALL cuts at allowed instants.  The one
    reading is real: `ONE_READING_GAP` below is a map on which the greedy plan is a reading longer than the optimum
    (the latest allowed instant in reach lies exactly at the limit, the next one a reading later, nothing for a whole
    limit after that: only a cut EARLIER than the latest one in reach gets past it, which the scan never tries);
  * feasibility of the greedy plan is monotone in the limit, which the device's 64-candidates-at-a-time search relies on.
"""
import numpy as np
import pytest

from helpers import tp_planner_reference as ref

# the shapes tests/test_tp_planner_gpu.py runs: readings per channel, and the pieces asked for
GPU_READINGS = (64, 65, 128, 129, 345)
GPU_PIECES = (2, 3, 8, 63)

# quiet 0..10 (instants 8, 9 allowed), 14..24 (22, 23), 37..47 (45, 46), loud elsewhere; 66 readings into at most 4 pieces.
# Optimum 22: cuts 9 | 23 | 45.  The greedy scan at limit 22 cuts at 22, from where only 23 is in reach: one reading
# away, too short a piece; at 23 it cuts 23 | 46.
ONE_READING_GAP = ([(0.0, 11), (1.0, 3), (0.0, 11), (1.0, 12), (0.0, 11), (1.0, 18)], 66, 4)


def energy_of(stretches, n_readings):
    e = ref.stretches_to_levels(stretches, n_readings).astype(np.float32)
    return e


def family():
    """(name, energy [NB] float32, K), seeded."""
    rng = np.random.default_rng(20240611)
    out = []
    for nb in GPU_READINGS:
        for k in GPU_PIECES:
            for rep in range(6):
                s = ref.random_stretches(rng, nb)
                e = energy_of(s, nb)
                if e.max() < 1.0:
                    e[int(np.argmax(e))] = 1.0
                out.append((f"random nb={nb} k={k} #{rep}", e, k))
            out.append((f"never quiet nb={nb} k={k}", (0.3 + 0.7 * rng.random(nb)).astype(np.float32), k))
            out.append((f"quiet throughout nb={nb} k={k}", np.zeros(nb, np.float32), k))
            # (faint but level: every reading is the loudest one, so none is quiet)
            out.append((f"never quiet, faint and level nb={nb} k={k}", np.full(nb, 0.00005, np.float32), k))
            for quiet_len in (5, 9):
                at = int(rng.integers(10, nb - 20))
                e = np.ones(nb, np.float32)
                e[at:at + quiet_len] = 0.01
                out.append((f"one quiet stretch of {quiet_len} nb={nb} k={k}", e, k))
            for quiet_len in (10, 11):           # the shortest that admit a cut: one instant, two instants
                at = int(rng.integers(10, nb - 20))
                e = np.ones(nb, np.float32)
                e[at:at + quiet_len] = 0.01
                out.append((f"one quiet stretch of {quiet_len} nb={nb} k={k}", e, k))
    for rep in range(400):
        nb, k = int(rng.integers(64, 201)), int(rng.integers(2, 13))
        e = energy_of(ref.random_stretches(rng, nb, loud=(3, 25), quiet=(8, 16)), nb)
        e[int(np.argmax(e))] = 1.0
        out.append((f"short stretches nb={nb} k={k} #{rep}", e, k))
    s, nb, k = ONE_READING_GAP
    out.append(("one-reading gap", energy_of(s, nb), k))
    return out


FAMILY = family()


def test_allowed_instants_by_definition():
    """The quiet window: 8 readings before to 1 after, all of them there, at most float32(0.08) x the loudest."""
    e = np.ones(40, np.float32)
    e[5:15] = np.float32(0.08)           # 10 readings at exactly the threshold: quiet (<=); one instant, 13
    e[20:29] = 0.0                       # 9: none
    e[30:40] = 0.0                       # 10 at the end: 38 would be it
    assert list(np.flatnonzero(ref.allowed_instants(e))) == [13, 38]
    e[39] = 1.0
    assert list(np.flatnonzero(ref.allowed_instants(e))) == [13]
    e[5] = np.nextafter(np.float32(0.08), np.float32(1))
    assert not ref.allowed_instants(e).any()
    z = np.zeros(12, np.float32)         # a silent channel: its loudest reading is 0, and 0 <= 0
    assert list(np.flatnonzero(ref.allowed_instants(z))) == [8, 9, 10]
    assert list(ref.latest_allowed(ref.allowed_instants(z))) == [-1] * 8 + [8, 9, 10, 10]


def test_family_has_what_it_must():
    names = [n for n, _, _ in FAMILY]
    forced = [ref.plan_cuts(e, k)[2] for _, e, k in FAMILY]
    assert sum(forced) >= 40 and len(FAMILY) - sum(forced) >= 500
    for nb in GPU_READINGS:
        for k in GPU_PIECES:
            assert any(f"random nb={nb} k={k} " in n for n in names)
    for n, e, k in FAMILY:
        ok = ref.allowed_instants(e)
        if n.startswith("never quiet") or "stretch of 5" in n or "stretch of 9" in n:
            assert not ok.any(), n
        if n.startswith("quiet throughout"):
            assert ok[ref.QUIET_BEFORE:len(e) - ref.QUIET_AFTER].all(), n
        if "stretch of 10" in n:
            assert ok.sum() == 1, n
        if "stretch of 11" in n:
            assert ok.sum() == 2, n


@pytest.mark.parametrize("part", range(8))
def test_greedy_plan_against_the_optimum(part):
    gaps = 0
    for name, e, k in FAMILY[part::8]:
        cuts, limit, forced = ref.plan_cuts(e, k)
        try:
            longest, opt = ref.check_cuts(e, k, cuts, forced)
        except AssertionError as err:
            raise AssertionError(f"{name}: {err}") from err
        assert longest <= limit, name
        if not forced:
            assert not ref.needs_forced_cuts(ref.latest_allowed(ref.allowed_instants(e)), k)
            gaps += longest - opt
    print(f"part {part}: {gaps} plans one reading above the optimum")


def test_the_one_reading_gap_is_real():
    """Keeps `opt + 1` honest: on this map the greedy plan IS one reading longer than the optimum."""
    s, nb, k = ONE_READING_GAP
    e = energy_of(s, nb)
    assert list(np.flatnonzero(ref.allowed_instants(e))) == [8, 9, 22, 23, 45, 46]
    cuts, limit, forced = ref.plan_cuts(e, k)
    assert not forced and (cuts, limit) == ([23, 46], 23)
    longest, opt = ref.check_cuts(e, k, cuts, forced)
    assert (longest, opt) == (23, 22)
    assert ref.longest_piece([9, 23, 45], nb) == 22          # the optimum's cuts: all allowed, four pieces


@pytest.mark.parametrize("part", range(4))
def test_feasibility_is_monotone_in_the_limit(part):
    for name, e, k in FAMILY[part::4]:
        lastq = ref.latest_allowed(ref.allowed_instants(e))
        forced = ref.needs_forced_cuts(lastq, k)
        fits = ref.feasible_limits(lastq, k, forced)
        lo = -(-len(e) // k)
        first = lo + int(np.argmax(fits[lo:]))
        assert fits[len(e)] and fits[first:].all(), (name, np.flatnonzero(~fits[first:]) + first)
        assert ref.plan_cuts(e, k)[1] == first


def test_boundaries_in_samples():
    """own_start, row0, nominal as documented: rounded down to the block length, the warm-up in front, left-over pieces
    parked empty at the last cut, the last piece open-ended."""
    s, nb, k = ONE_READING_GAP
    e = energy_of(s, nb)
    own, row0, nominal, (cuts, _, _) = ref.boundaries(e, 6, 36, 1728)
    assert cuts == [23, 46]
    p1, p2 = 23 * 256 - (23 * 256) % 36, 46 * 256 - (46 * 256) % 36
    assert list(own) == [0, p1, p2, p2, p2, p2]
    assert list(row0) == [0, p1 - 1728, p2 - 1728, p2 - 1728, p2 - 1728, p2 - 1728]
    assert list(nominal) == [-(-p1 // 36), -(-(p2 - p1 + 1728) // 36), 48, 48, 48, ref.NO_NOMINAL]
    own, row0, _, _ = ref.boundaries(e, 6, 36, 6000)          # a warm-up longer than what lies in front: from the call's start
    assert list(row0) == [0, 0, p2 - 6000, p2 - 6000, p2 - 6000, p2 - 6000]


def test_workgroup_order_and_pairing():
    perm = np.arange(6 * 64)
    blocks, length = np.array([10, 11, 12, 13, 14, 15]), np.array([5, 9, 5, 7, 9, 1])
    p2, w2 = ref.workgroup_order(perm, blocks, length, pairs=False)      # ranks: 1, 4 (tie by position), 3, 0, 2, 5
    assert list(p2[::64] // 64) == [1, 4, 3, 0, 2, 5] and list(w2) == [11, 14, 13, 10, 12, 15]
    p2, w2 = ref.workgroup_order(perm, blocks, length, pairs=True)       # rank r beside rank 5 - r
    assert list(p2[::64] // 64) == [1, 5, 4, 2, 3, 0] and list(w2) == [11, 15, 14, 12, 13, 10]
    p2, _ = ref.workgroup_order(perm[:5 * 64], blocks[:5], length[:5], pairs=True)      # an odd count is not paired
    assert list(p2[::64] // 64) == [1, 4, 3, 0, 2]


def test_final_column_follows_the_chain():
    none = ref.NO_HANDOVER
    own = np.array([[0, 0], [1000, 1000], [1000, 2000], [3000, 2000]], np.int64)      # [K, C]
    hand = np.array([[500 + 1000, none], [none, none], [500 + 3000, none], [none, none]], np.uint64)
    # channel 0: chunk 0 hands over at 1000 (relative): the LAST chunk that begins by then is 2 (parked beside 1); 2 hands
    # over at 3000: chunk 3, which never does.  Channel 1: chunk 0 ran to the end.
    assert list(ref.final_columns(hand, own, 500)) == [3 * 2 + 0, 0 * 2 + 1]
    hand[0, 0] = 500 + 999               # before any later chunk's range: the chain ends where it began
    assert list(ref.final_columns(hand, own, 500)) == [0, 1]
