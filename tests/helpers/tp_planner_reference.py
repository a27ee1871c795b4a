"""A plain reference of the time-parallel planning chain (same_kernels.hip: tp_scout_kernel, tp_boundaries_kernel,
tp_sort_kernel, tp_align_kernel, tp_wg_order_kernel, chunk_final_column_pc_kernel): numpy and Python loops over one
channel, one column, one workgroup at a time.  Written from what the kernels' comments and DESIGN.md 4.6 say they
compute, so that tests/test_tp_planner_cpu.py can hold the ALGORITHM to an exhaustive optimum and
tests/test_tp_planner_gpu.py can hold the KERNELS to this file.

Units: a "reading" is the scout's energy over one block of SCOUT_BLOCK samples; cuts are counted in readings, own_start
and row0 in samples, nominal and the workgroups' figures in blocks of the demodulation kernel (block_len samples).
"""
import numpy as np

SCOUT_BLOCK = 256          # samples per reading; the scout adds up the magnitudes of the first SCOUT_SECTOR of them
SCOUT_SECTOR = 16
QUIET_BEFORE = 8           # an instant is allowed when the channel was quiet from 8 readings before it (2 048 samples) ...
QUIET_AFTER = 1            # ... to one reading after it
QUIET_RATIO = np.float32(0.08)     # "quiet": at most 8 % of the channel's loudest reading
MIN_READINGS = 2           # the shortest piece
WAVE = 64                  # grid positions per workgroup of the demodulation launch
SORT_BUCKETS = 4096        # the sort's buckets, SORT_BUCKET_BLOCKS blocks of length each, longest first
SORT_BUCKET_BLOCKS = 4
NO_NOMINAL = 0xFFFFFFFF    # the last piece ends with the input
NO_HANDOVER = 0xFFFFFFFFFFFFFFFF


# ---- scout ------------------------------------------------------------------------------------------------------------
def scout(x, n_readings):
    """x [C, in_samples] float32 -> energy [C, n_readings] float32: reading (c, j) is the sum of the magnitudes of the first
    16 samples of block j, four groups of four added pairwise, each addition rounded to float32."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] >= n_readings * SCOUT_BLOCK
    a = np.abs(x[:, :n_readings * SCOUT_BLOCK].reshape(x.shape[0], n_readings, SCOUT_BLOCK)[:, :, :SCOUT_SECTOR])
    four = [(a[:, :, 4 * q] + a[:, :, 4 * q + 1]) + (a[:, :, 4 * q + 2] + a[:, :, 4 * q + 3]) for q in range(4)]
    e = (four[0] + four[1]) + (four[2] + four[3])
    assert e.dtype == np.float32
    return e


# ---- allowed instants -------------------------------------------------------------------------------------------------
def allowed_instants(e):
    """e [NB] float32 -> bool [NB]: reading j may carry a cut."""
    e = np.asarray(e, np.float32)
    nb = len(e)
    thr = np.float32(QUIET_RATIO * e.max()) if nb else np.float32(0)
    ok = np.zeros(nb, bool)
    for j in range(QUIET_BEFORE, nb - QUIET_AFTER):
        ok[j] = bool(np.all(e[j - QUIET_BEFORE:j + QUIET_AFTER + 1] <= thr))
    return ok


def latest_allowed(ok):
    """lastq [NB]: the latest allowed instant at or before j, -1 where there is none."""
    out, run = np.empty(len(ok), np.int64), -1
    for j, a in enumerate(ok):
        if a:
            run = j
        out[j] = run
    return out


# ---- boundaries -------------------------------------------------------------------------------------------------------
def greedy_cuts(lastq, k_max, limit, forced):
    """The cuts of the greedy plan for pieces of at most `limit` readings, or None when it needs more than k_max pieces or
    gets stuck.  It always cuts at the latest allowed instant in reach; `forced`: where none is, at the limit itself."""
    nb = len(lastq)
    cuts, pos = [], 0
    while nb - pos > limit:
        q = int(lastq[min(pos + limit, nb - 1)])
        if q < pos + MIN_READINGS:
            if not forced:
                return None
            q = pos + limit
        q = min(q, nb - MIN_READINGS)
        if q <= pos:
            return None
        cuts.append(q)
        pos = q
        if len(cuts) + 1 > k_max:
            return None
    return cuts


def needs_forced_cuts(lastq, k_max):
    return greedy_cuts(lastq, k_max, len(lastq) - 1, False) is None


def feasible_limits(lastq, k_max, forced):
    """bool [NB + 1]: whether the greedy plan fits k_max pieces at limit L (index L; below the search's floor: False)."""
    nb = len(lastq)
    out = np.zeros(nb + 1, bool)
    for limit in range(-(-nb // k_max), nb + 1):
        out[limit] = greedy_cuts(lastq, k_max, limit, forced) is not None
    return out


def plan_cuts(e, k_max):
    """(cuts, limit, forced) of one channel: the greedy plan at the smallest limit in [ceil(NB / K), NB] that fits, found
    by trying them one after the other."""
    lastq = latest_allowed(allowed_instants(e))
    nb = len(lastq)
    forced = needs_forced_cuts(lastq, k_max)
    for limit in range(-(-nb // k_max), nb + 1):
        cuts = greedy_cuts(lastq, k_max, limit, forced)
        if cuts is not None:
            return cuts, limit, forced
    raise AssertionError("the whole call as one piece always fits")


def longest_piece(cuts, nb):
    edges = [0] + list(cuts) + [nb]
    return max(b - a for a, b in zip(edges, edges[1:]))


def optimal_longest_piece(ok, k_max):
    """The shortest possible longest piece over ALL ways to cut [0, NB) at allowed instants into at most k_max pieces of at
    least MIN_READINGS readings -- independent of the greedy scan: for a limit L, need[p] is the fewest pieces that end
    with a cut at p (dynamic programme over every earlier cut in [p - L, p - MIN_READINGS]); the smallest L that fits is
    found by bisection, which is sound here because a plan that respects L respects L + 1."""
    ok = np.asarray(ok, bool)
    nb = len(ok)
    big = 1 << 30

    def fits(limit):
        need = np.full(nb + 1, big, np.int64)      # need[p]: pieces in front of a cut at p (need[0] = 0: the call's start)
        need[0] = 0
        for p in range(MIN_READINGS, nb):
            if ok[p]:
                lo = max(0, p - limit)
                best = need[lo:p - MIN_READINGS + 1].min()
                if best < big:
                    need[p] = best + 1
        lo = max(0, nb - limit)
        hi = nb - MIN_READINGS
        return hi >= lo and need[lo:hi + 1].min() + 1 <= k_max

    lo, hi = 1, nb
    if not fits(hi):
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if fits(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def boundaries(e, k_max, block_len, warmup_samples):
    """own_start, row0 (before alignment), nominal [K] of one channel, and (cuts, limit, forced)."""
    cuts, limit, forced = plan_cuts(e, k_max)
    used = len(cuts) + 1

    def own(k):
        # pieces that are left over sit, empty, at the last cut; the piece after it is the last chunk
        i = min(k, used - 1)
        p = cuts[i - 1] * SCOUT_BLOCK if k >= 1 and i >= 1 else 0
        return p - p % block_len

    own_start = np.array([own(k) for k in range(k_max)], np.int64)
    row0 = np.array([0 if k == 0 or own_start[k] < warmup_samples else own_start[k] - warmup_samples for k in range(k_max)], np.int64)
    nominal = np.array([-(-(own_start[k + 1] - row0[k]) // block_len) if k + 1 < k_max else NO_NOMINAL for k in range(k_max)], np.int64)
    return own_start, row0, nominal, (cuts, limit, forced)


def plan_boundaries(energy, k_max, block_len, warmup_samples):
    """The same for every channel: own_start, row0, nominal as [K, C] (column v = k * C + c), and the per-channel details."""
    n_ch = energy.shape[0]
    own_start, row0, nominal = (np.zeros((k_max, n_ch), np.int64) for _ in range(3))
    details = []
    for c in range(n_ch):
        own_start[:, c], row0[:, c], nominal[:, c], d = boundaries(energy[c], k_max, block_len, warmup_samples)
        details.append(d)
    return own_start, row0, nominal, details


def cuts_of_own_start(own_start_c):
    """The cuts, in readings, behind one channel's own_start [K] (rounded down to the block length, less than a reading),
    the parked pieces' repeats dropped."""
    cuts = []
    for p in own_start_c[1:]:
        q = (int(p) + SCOUT_BLOCK - 1) // SCOUT_BLOCK
        if q and (not cuts or q != cuts[-1]):
            cuts.append(q)
    return cuts


def check_cuts(e, k, cuts, forced):
    """The properties of a plan's cuts (in readings) on energy map e; returns (longest, opt) -- opt None when forced."""
    nb = len(e)
    ok = allowed_instants(e)
    edges = [0] + list(cuts) + [nb]
    assert len(cuts) + 1 <= k, ("too many pieces", cuts)
    assert nb - edges[-2] >= MIN_READINGS or not cuts, ("the last cut is too late", cuts)
    longest = longest_piece(cuts, nb)
    if forced:
        # (a forced cut falls where the limit puts it, held back to NB - 2: the piece in front of that one may be a single
        # reading -- 65 readings into 63 pieces are 2, 2, ... 2, 1, 2)
        assert all(b > a for a, b in zip(edges, edges[1:])), ("an empty or backward piece", cuts)
        return longest, None
    assert all(b - a >= MIN_READINGS for a, b in zip(edges, edges[1:])), ("a piece is too short", cuts)
    assert all(ok[q] for q in cuts), ("a cut at an instant that is not allowed", cuts, np.flatnonzero(ok))
    opt = optimal_longest_piece(ok, k)
    assert opt is not None and opt <= longest <= opt + 1, (longest, opt, cuts)
    return longest, opt


# ---- sort -------------------------------------------------------------------------------------------------------------
def sort_keys(row0, nominal, n_ch, k_max, block_len, whole_samples):
    """(group, bucket) of every column from row0 BEFORE alignment: group 0 the last chunk, 1 chunk 0, 2 the rest; the
    bucket falls with the column's length (its whole run for a last chunk, else what it is to own with its warm-up)."""
    row0, nominal = np.asarray(row0).reshape(-1), np.asarray(nominal).reshape(-1)
    group, bucket = np.zeros(k_max * n_ch, np.int64), np.zeros(k_max * n_ch, np.int64)
    for v in range(k_max * n_ch):
        chunk = v // n_ch
        avail = (whole_samples - int(row0[v])) // block_len
        group[v] = 0 if chunk == k_max - 1 else (1 if chunk == 0 else 2)
        length = avail if group[v] == 0 else min(int(nominal[v]), avail)
        bucket[v] = SORT_BUCKETS - 1 - min(length // SORT_BUCKET_BLOCKS, SORT_BUCKETS - 1)
    return group, bucket


def check_sorted_perm(perm, group, bucket, n_ch, k_max):
    """What a sorted perm must be whatever order the atomics landed in: a permutation; the last chunk's columns at grid
    positions 0 .. C-1 in channel order; chunk 0's at C .. 2C-1 and the rest behind, each by ascending bucket."""
    perm = np.asarray(perm, np.int64)
    n = n_ch * k_max
    assert perm.shape == (n,)
    assert np.array_equal(np.sort(perm), np.arange(n)), "perm is no permutation"
    assert np.array_equal(perm[:n_ch], (k_max - 1) * n_ch + np.arange(n_ch)), "last chunk out of channel order"
    first = perm[n_ch:2 * n_ch]
    assert np.all(group[first] == 1), "grid positions C .. 2C-1 are not chunk 0's"
    assert np.all(np.diff(bucket[first]) >= 0), "chunk 0 not by ascending bucket"
    rest = perm[2 * n_ch:]
    assert np.all(group[rest] == 2)
    assert np.all(np.diff(bucket[rest]) >= 0), "middle chunks not by ascending bucket"


# ---- align and workgroup order, given the device's own perm -------------------------------------------------------------
def align(perm, row0, nominal, n_ch, k_max, block_len, whole_samples):
    """(wg_blocks [W], row0 after alignment [K * C], wg_len [W]): a workgroup runs as many blocks as its lane with the most
    input left; the lanes of a last-chunk workgroup all start at that lane's row, so that they end with the input; its
    length if every lane hands over on time is that of its longest lane."""
    perm = np.asarray(perm, np.int64)
    before = np.asarray(row0, np.int64).reshape(-1)
    nominal = np.asarray(nominal, np.int64).reshape(-1)
    after = before.copy()
    n_wg = len(perm) // WAVE
    wg_blocks, wg_len = np.zeros(n_wg, np.int64), np.zeros(n_wg, np.int64)
    for w in range(n_wg):
        cols = perm[w * WAVE:(w + 1) * WAVE]
        avail = [(whole_samples - int(before[v])) // block_len for v in cols]
        m = max(avail)
        wg_blocks[w] = m
        lens = []
        for v, a in zip(cols, avail):
            if v // n_ch == k_max - 1:
                after[v] = whole_samples - m * block_len
                lens.append(m)
            else:
                lens.append(min(int(nominal[v]), a))
        wg_len[w] = max(lens)
    return wg_blocks, after, wg_len


def workgroup_order(perm, wg_blocks, wg_len, pairs):
    """(perm2, wg2_blocks): the workgroups longest first, ties by position; `pairs` and an even count: rank r and rank
    n - 1 - r next to each other, the longer of the two first."""
    n = len(wg_len)
    order = sorted(range(n), key=lambda w: (-int(wg_len[w]), w))
    perm2, wg2 = np.zeros(n * WAVE, np.int64), np.zeros(n, np.int64)
    for rank, w in enumerate(order):
        pos = rank
        if pairs and n % 2 == 0:
            pos = 2 * rank if rank < n // 2 else 2 * (n - 1 - rank) + 1
        perm2[pos * WAVE:(pos + 1) * WAVE] = perm[w * WAVE:(w + 1) * WAVE]
        wg2[pos] = wg_blocks[w]
    return perm2, wg2


# ---- the column a channel's state is taken from -------------------------------------------------------------------------
def final_columns(handover, own_start, counter0):
    """handover, own_start [K, C]: follow the hand-over chain from chunk 0 -- a column that handed over at instant h is
    followed by the LAST later chunk whose own range begins at or before h -- to the chunk it ends in."""
    k_max, n_ch = own_start.shape
    out = np.zeros(n_ch, np.int64)
    for c in range(n_ch):
        cur = 0
        while True:
            h = int(handover[cur, c])
            if h == NO_HANDOVER:
                break
            later = [k for k in range(cur + 1, k_max) if counter0 + int(own_start[k, c]) <= h]
            if not later:
                break
            cur = later[-1]
        out[c] = cur * n_ch + c
    return out


# ---- energy maps for the tests ----------------------------------------------------------------------------------------
def stretches_to_levels(stretches, n_readings):
    """[(level, length), ...] -> level per reading [n_readings] (the last stretch runs to the end, or is cut there)."""
    out = np.zeros(n_readings, np.float64)
    j = 0
    for level, length in stretches:
        out[j:j + length] = level
        j += length
        if j >= n_readings:
            break
    if j < n_readings:
        out[j:] = stretches[-1][0]
    return out


def random_stretches(rng, n_readings, loud=(5, 40), quiet=(3, 30)):
    """Loud and quiet stretches in turn, random lengths, until n_readings are covered.  Quiet levels lie at or below 7 % of
    the loudest (1.0), loud ones at or above 9 %."""
    out, j, is_loud = [], 0, bool(rng.integers(2))
    while j < n_readings:
        if is_loud:
            level, length = float(rng.choice([1.0, 0.6, 0.3, 0.09])), int(rng.integers(loud[0], loud[1] + 1))
        else:
            level, length = float(rng.choice([0.0, 0.001, 0.03, 0.07])), int(rng.integers(quiet[0], quiet[1] + 1))
        out.append((level, length))
        j += length
        is_loud = not is_loud
    return out
