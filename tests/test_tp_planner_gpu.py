"""The six planning kernels of a channel-major time-parallel call (same_kernels.hip: tp_scout_kernel, tp_boundaries_kernel,
tp_sort_kernel, tp_align_kernel, tp_wg_order_kernel, chunk_final_column_pc_kernel) against the plain reference of
helpers/tp_planner_reference.py, through the read-back of the last launch's plan (same_batch_debug_tp_plan).

The decode contract (tests/test_time_parallel.py) forgives a bad plan -- a chunk cut inside a burst runs on, an empty piece
hands over at once -- so no case here asserts it.  What is asserted is what the kernels WRITE:
  * the energy map, bit for bit (the reference adds in the kernel's order, nothing in it is fused);
  * own_start, row0 and nominal, equal to the reference's plan for the device's own energy map;
  * on the device's cuts directly: allowed instants, at most K pieces, within one reading of the exhaustive optimum
    (tests/test_tp_planner_cpu.py shows that the one reading is real), feasibility monotone in the limit;
  * perm: the identity in grid order; sorted, a permutation with the groups where they belong and ascending buckets
    (the order inside a bucket is the atomics');
  * given the device's perm: the workgroups' block counts, the last chunk's common first rows, the workgroups' lengths,
    their order longest first (ties by position) or paired long with short, perm2;
  * given the device's hand-over records: the column every channel's state is taken from.

Inputs are made so that a wrong kernel shows: every sample random (a scout reading another sector, channel or pitch
reads other numbers), negative values and -0.0, per channel its own loud and quiet stretches with levels on both sides
of the 8 % threshold (7 % and 9 % of the loudest reading), channels that are never quiet (forced cuts) and channels that
are silent (loudest reading 0: every instant allowed), quiet stretches of exactly 9, 10 and 11 readings (10 is the
shortest that admits a cut).  With 65 readings and more a lane of the planner scans several readings, and the quiet
stretches straddle those lanes' borders."""
import numpy as np
import pytest

from helpers import tp_planner_reference as ref

pytestmark = pytest.mark.gpu

RATE = 22050
BLOCK_LEN = 36          # the symbol-paced pipeline's, which runs the chunks of these batches (asserted, not assumed)


@pytest.fixture(scope="module")
def sa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sameold_amd import build as sbuild
    sbuild.build()
    import sameold_amd
    sameold_amd.load_library()
    return sameold_amd


def call_length(n_readings):
    """Samples per channel of a call whose whole blocks hold exactly n_readings readings: a multiple of 4 (16-byte
    streams), of neither the block length nor the scout's 256."""
    whole = -(-n_readings * ref.SCOUT_BLOCK // BLOCK_LEN) * BLOCK_LEN
    n = whole + 4
    assert n % 4 == 0 and n % BLOCK_LEN != 0 and n % ref.SCOUT_BLOCK != 0
    assert (n - n % BLOCK_LEN) // ref.SCOUT_BLOCK == n_readings
    return n


def channel_levels(rng, c, nb):
    """The level of every reading of channel c, as a fraction of the channel's loudest (1.0)."""
    kind = c % 8
    if kind == 0:                                                  # never quiet: forced cuts
        lv = 0.3 + 0.7 * rng.random(nb)
    elif kind == 1:                                                # silent: every instant allowed
        return np.zeros(nb)
    elif kind == 2:                                                # quiet for exactly 9, 10 and 11 readings, at random places
        gaps = rng.multinomial(nb - 30 - 12, [0.25] * 4) + 3
        s = [(1.0, gaps[0]), (0.01, 9), (0.5, gaps[1]), (0.0, 10), (0.8, gaps[2]), (0.03, 11), (0.6, gaps[3])]
        lv = ref.stretches_to_levels(s, nb)
    elif kind == 3:                                                # 9 % is loud, 7 % is quiet
        s = [(1.0, int(rng.integers(2, 6))), (0.09, 14), (0.7, 3), (0.07, 14), (0.4, 3)] + ref.random_stretches(rng, nb)
        lv = ref.stretches_to_levels(s, nb)
    else:
        lv = ref.stretches_to_levels(ref.random_stretches(rng, nb, loud=(3, 30), quiet=(6, 24)), nb)
    loud = np.flatnonzero(lv >= 0.09)
    lv[rng.choice(loud) if len(loud) else 0] = 1.0
    return lv


def make_input(seed, n_ch, nb, n_call):
    """x [n_ch, n_call] float32 on the CPU.  The first 16 samples of every reading's block add up, in magnitude, to
    8 x its level (to float32 rounding); everything else is as random, at the same level."""
    rng = np.random.default_rng(seed)
    levels = np.stack([channel_levels(rng, c, nb) for c in range(n_ch)]).astype(np.float32)
    def noise(shape):
        u = np.float32(0.25) + np.float32(0.75) * rng.random(shape, dtype=np.float32)
        return u * np.where(rng.random(shape, dtype=np.float32) < 0.5, np.float32(-1), np.float32(1))

    body = noise((n_ch, nb, ref.SCOUT_BLOCK))
    sector = body[:, :, :ref.SCOUT_SECTOR]                         # (a view)
    sector *= (8.0 / np.abs(sector).sum(axis=2, dtype=np.float64))[:, :, None].astype(np.float32)
    body *= levels[:, :, None]                                     # (a level of 0 leaves zeros of both signs)
    tail = np.float32(0.01) * noise((n_ch, n_call - nb * ref.SCOUT_BLOCK))
    x = np.ascontiguousarray(np.concatenate([body.reshape(n_ch, -1), tail], axis=1))
    assert x.dtype == np.float32 and x.shape == (n_ch, n_call)
    assert (x < 0).any() and (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
    return x


def run_call(sa, rx, x):
    import torch
    xd = torch.from_numpy(x).cuda()
    rx.process_tensor(xd, layout=sa.LAYOUT_CHANNEL_MAJOR)
    rx.sync()
    assert rx.time_parallel_per_channel(), "the call did not take the per-channel path"
    return rx.debug_tp_plan()


def check_plan(p, x, k_asked, sort, counter0=0):
    """Everything the planning kernels wrote for one launch, against the reference.  Returns figures for the test's log."""
    n_ch, n_call = x.shape
    K, bl, warm, whole, nb = p["n_chunks"], p["block_len"], p["warmup_samples"], p["whole_samples"], p["scout_blocks"]
    cols, n_wg = K * n_ch, K * n_ch // ref.WAVE
    # the plan's scalars: what the call was, not what the code's rules make of it
    assert (p["channels"], p["in_samples"], p["counter0"]) == (n_ch, n_call, counter0)
    assert bl == BLOCK_LEN and whole == n_call - n_call % bl and whole != n_call and nb == whole // ref.SCOUT_BLOCK
    assert K == k_asked and 0 < warm and warm % bl == 0
    assert (p["sort_mode"], p["lpt"], p["pair_groups"]) == {0: (0, 0, 0), 1: (1, 1, 0), 2: (0, 1, 1)}[sort]
    g = p["geom"].astype(np.int64)
    assert p["w_total"] == len(g) and p["w_perm2"] + cols <= len(g)

    def words(name, n):
        return g[p["w_" + name]:p["w_" + name] + n]

    # scout: bit for bit
    energy = p["energy"]
    want = ref.scout(x, nb)
    assert energy.shape == want.shape == (n_ch, nb)
    bad = np.argwhere(energy.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} readings differ, first (channel, reading) {bad[0]}: {energy[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}"

    # boundaries, from the device's own map
    own_ref, row0_ref, nom_ref, details = ref.plan_boundaries(energy, K, bl, warm)
    own, row0, nominal = words("own_start", cols).reshape(K, n_ch), words("row0", cols).reshape(K, n_ch), words("nominal", cols).reshape(K, n_ch)
    for name, got, exp in (("own_start", own, own_ref), ("nominal", nominal, nom_ref), ("row0", row0[:K - 1], row0_ref[:K - 1])):
        bad = np.argwhere(got != exp)
        assert len(bad) == 0, f"{name}: {len(bad)} differ, first (chunk, channel) {bad[0]}: {got[tuple(bad[0])]} for {exp[tuple(bad[0])]}"
    assert np.all(own % bl == 0) and np.all(row0 % bl == 0) and np.all(np.diff(own, axis=0) >= 0) and np.all(own[0] == 0)

    # the device's cuts themselves
    n_forced = n_gap = n_parked = 0
    for c in range(n_ch):
        cuts = ref.cuts_of_own_start(own[:, c])
        forced = details[c][2]
        lastq = ref.latest_allowed(ref.allowed_instants(energy[c]))
        try:
            longest, opt = ref.check_cuts(energy[c], K, cuts, forced)
            fits = ref.feasible_limits(lastq, K, forced)
            first = int(np.argmax(fits))
            assert fits[first:].all(), ("feasibility is not monotone in the limit", np.flatnonzero(~fits[first:]) + first)
            assert longest <= first, ("longer than the smallest feasible limit", longest, first)
        except AssertionError as err:
            raise AssertionError(f"channel {c}: {err}") from err
        n_forced += forced
        n_gap += 0 if forced else longest - opt
        n_parked += len(cuts) + 1 < K

    # sort
    perm = words("perm", cols)
    if p["sort_mode"]:
        group, bucket = ref.sort_keys(row0_ref, nom_ref, n_ch, K, bl, whole)
        ref.check_sorted_perm(perm, group, bucket, n_ch, K)
    else:
        assert np.array_equal(perm, np.arange(cols))

    # align and workgroup order, given that perm
    wg_ref, row0_after, len_ref = ref.align(perm, row0_ref, nom_ref, n_ch, K, bl, whole)
    assert np.array_equal(words("wg", n_wg), wg_ref)
    assert np.array_equal(row0.reshape(-1), row0_after), "row0 after alignment"
    assert np.all(row0[K - 1] <= row0_ref[K - 1])
    if p["lpt"]:
        perm2_ref, wg2_ref = ref.workgroup_order(perm, wg_ref, len_ref, bool(p["pair_groups"]))
        assert np.array_equal(words("wg2", 2 * n_wg)[n_wg:], len_ref), "wg_len"
        assert np.array_equal(words("wg2", n_wg), wg2_ref), "wg2"
        assert np.array_equal(words("perm2", cols), perm2_ref), "perm2"

    # the column every channel's state is taken from.  (These inputs carry no burst, so every column hands over and every
    # chain ends in the last chunk; what the walk has to get right here is which of several pieces parked at one instant
    # follows -- the last -- and the call's first sample in front of own_start.  A chain that ends early is the reference's
    # own test: tests/test_tp_planner_cpu.py.)
    assert p["handover"].shape == (K, n_ch)
    final_ref = ref.final_columns(p["handover"], own, counter0)
    assert np.array_equal(p["final_col"].astype(np.int64), final_ref)
    handed = int((p["handover"] != np.uint64(ref.NO_HANDOVER)).sum())
    assert handed >= n_ch, "no chain to follow: no column handed over"
    return dict(forced=n_forced, one_reading_above=n_gap, parked=n_parked, handed_over=handed,
                final_in_last_chunk=int((final_ref // n_ch == K - 1).sum()), workgroups=n_wg)


# readings per channel, channels, pieces, SAME_TP_SORT.  63 pieces are the most a per-channel call takes: they are more
# than the call has cuts for, so pieces are left over and parked.  SAME_TP_SORT=2: 63 workgroups are not paired, 8 are.
CASES = [(64, 64, 2, 0), (65, 64, 3, 1), (128, 192, 8, 0), (129, 64, 63, 1), (345, 192, 8, 1), (345, 64, 63, 0),
         (64, 64, 63, 2), (128, 64, 8, 2), (65, 192, 3, 2), (129, 192, 2, 1), (345, 64, 3, 0)]


def make_batch(sa, monkeypatch, n_ch, k, sort):
    monkeypatch.setenv("SAME_PIPE_LANES", "64")          # (small test batches would otherwise get 16-channel workgroups)
    monkeypatch.setenv("SAME_TP_SORT", str(sort))
    monkeypatch.delenv("SAME_RELAXED", raising=False)    # relaxed arithmetic in the chunks: the mode's default
    rx = sa.SameReceiverBuilder(RATE).build_batch(n_ch, time_parallel=True)
    rx.time_parallel_config(max_chunks=k, min_own_samples=BLOCK_LEN)      # (so that calls this short are still cut)
    return rx


@pytest.mark.parametrize("nb,n_ch,k,sort", CASES)
def test_planning_kernels_against_the_reference(sa, monkeypatch, nb, n_ch, k, sort):
    n_call = call_length(nb)
    x = make_input(7000 + 13 * nb + n_ch + 101 * k + sort, n_ch, nb, n_call)
    rx = make_batch(sa, monkeypatch, n_ch, k, sort)
    p = run_call(sa, rx, x)
    seen = check_plan(p, x, k, sort)
    print(f"nb={nb} C={n_ch} K={k} sort={sort}: {seen}")
    # the inputs did what they were made for
    assert seen["forced"] >= n_ch // 8, "the never-quiet channels took no forced cuts"
    if k == 63:
        assert seen["parked"] == n_ch, "63 pieces must leave some over on every channel"


def test_each_read_back_belongs_to_its_own_call(sa, monkeypatch):
    """Two streaming calls, one on either launch slot (the geometry and the hand-over records are the slot's, the energy map
    and the final columns one buffer for both): each read-back is its own call's.  And no stale plan comes back once a
    launch without one has run."""
    nb, n_ch, k = 128, 64, 8
    n_call = call_length(nb)
    rx = make_batch(sa, monkeypatch, n_ch, k, 1)
    with pytest.raises(sa.SameError):
        rx.debug_tp_plan()                                 # no launch yet
    xs = [make_input(8100 + i, n_ch, nb, n_call) for i in range(3)]
    plans = []
    for i, x in enumerate(xs):
        p = run_call(sa, rx, x)
        print(f"call {i}: {check_plan(p, x, k, 1, counter0=i * n_call)}")
        plans.append(p)
    assert not np.array_equal(plans[0]["energy"], plans[1]["energy"])
    assert not np.array_equal(plans[0]["geom"][:k * n_ch], plans[1]["geom"][:k * n_ch])
    # a call too short to be cut runs as an ordinary launch: there is no plan to read
    import torch
    short = torch.from_numpy(np.ascontiguousarray(xs[0][:, :4096])).cuda()
    rx.process_tensor(short, layout=sa.LAYOUT_CHANNEL_MAJOR)
    rx.sync()
    assert not rx.time_parallel_per_channel()
    with pytest.raises(sa.SameError):
        rx.debug_tp_plan()
