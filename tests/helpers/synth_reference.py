"""Float64 reference of the two signal generators of sameold_amd/csrc/same_synth.hip, numpy only.

Written from the generators' documented definition -- the header comment and the comment over the trial generator in
same_synth.hip, include/same_rx.h ("helpers") and DESIGN.md section 5 -- and not by transcribing the kernels: everything
here is whole-array numpy over [T, channels] and nothing is a per-sample loop.  What those texts leave open and only the
seeded draws can settle is listed here, so that this file is the place where it is written down:

  streams   header text of channel c: splitmix64 from  seed ^ 0xd1b54a32d192ed03 * ((c + 1) mod 2^32);  draws in order:
            originator (mod 4 into EAS CIV WXR PEP), event (3 letters, base 26, least significant first), location count
            (1 + mod 6), one draw per location (6 digits, base 10, least significant first), one draw for +TTTT and, from
            the digits that follow, JJJHHMM, one draw for the 8 station characters (base 37 into A-Z 0-9 /).
            parameters of channel c: splitmix64 from  seed ^ 0x2545f4914f6cdd1d * ((c + 1) mod 2^32).
            workload draws: lead (mod 1 000 000 microseconds), amplitude (mod 65 536), skew (mod 2 001).
            trial draws:    amplitude (mod 65 536), skew (mod 2 001), lead fraction (mod 65 536, of one symbol).
            workload noise of channel c: splitmix64 from  seed * 0x9e3779b97f4a7c15 + c * 0x632be59bd9b4e019,  one draw
            per sample (whether or not the sample is in a burst); u1 = (bits 40..63 + 1) / 2^24 in (0, 1], u2 = bits
            8..31 / 2^24 in [0, 1), g = sqrt(-2 ln u1) cos(2 pi u2).  (The kernel writes u1's divisor as 16777217.0f,
            which is 2^24 in float32: 16 777 217 has no float32 of its own.)
            trial noise: Philox4x32-10, key = (seed low word, seed high word), counter = (block low word, block high
            word, trial, 0x5a4d4531) with block = sample // 4; of the four output words, (w0, w1) and (w2, w3) are the
            (u1, u2) of one Box-Muller draw each, u1 = ((w >> 8) + 1) / 2^24, u2 = (w >> 8) / 2^24, and samples 4b .. 4b+3
            are  r0 cos, r0 sin, r1 cos, r1 sin.
  Eb/N0     sigma = A sqrt(sps / (4 Eb/N0)) uses the nominal sps = fs / 520.83, i.e. Eb is the energy of a bit of nominal
            length, whatever the trial's own clock skew.
  wrap      the trial number first_trial + c and the stream index c + 1 are 32-bit and wrap.

The phase is accumulated exactly in uint32 and the cosine is evaluated in float64 on the phase as rounded to float32 (the
documented `(float)phase` step); that rounding is the only single-precision step imitated here.  Amplitude, sigma, exp10,
sqrt, log, and cos/sin of 2 pi u2 are float64.  Arguments that cross the C ABI as `float` (Eb/N0 grid, noise_sigma) are
taken at their float32 value, since that is the number the generator is given.

Philox known answers (KAT_PHILOX4X32_10): the three philox4x32 10-round lines of Random123's kat_vectors (Salmon, Moraes,
Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter and key all zero, all ones, and the digits of
pi.  They were written down from memory and then checked, together with philox4x32_10 below, against a second
implementation: the philox_engine of PyTorch's ATen/core/PhiloxRNGEngine.h, compiled as a stand-alone host program, gives
the same twelve words for the same three inputs.
"""
import numpy as np

MASK64 = (1 << 64) - 1
MASK32 = (1 << 32) - 1
BAUD = 520.83
MARK_HZ, SPACE_HZ = 2083.3, 1562.5
PREAMBLE_BYTES = 16
EOM = b"NNNN"

# (counter, key, output)
KAT_PHILOX4X32_10 = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ------------------------------------------------------------------ integer generators
def splitmix64(state):
    """one step of SplitMix64 on a Python int: (new state, output)"""
    state = (state + 0x9e3779b97f4a7c15) & MASK64
    z = state
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK64
    return state, z ^ (z >> 31)


class _Stream:
    def __init__(self, state):
        self.state = state & MASK64

    def __call__(self):
        self.state, out = splitmix64(self.state)
        return out


def _splitmix64_at(start, steps):
    """outputs number steps[...] (1 = the first) of the stream that starts at start[...]; np.uint64, wrapping"""
    with np.errstate(over="ignore"):
        z = start + steps * np.uint64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))


def payload(seed, channel):
    """header text the generators transmit on `channel`: ZCZC-ORG-EEE(-PSSCCC){1..6}+TTTT-JJJHHMM-LLLLLLLL-"""
    rnd = _Stream((seed & MASK64) ^ (0xd1b54a32d192ed03 * ((channel + 1) & MASK32)))
    out = "ZCZC-" + ("EAS", "CIV", "WXR", "PEP")[rnd() % 4] + "-"
    r = rnd()
    for _ in range(3):
        out += chr(ord("A") + r % 26)
        r //= 26
    for _ in range(1 + rnd() % 6):
        r = rnd()
        out += "-"
        for _ in range(6):
            out += chr(ord("0") + r % 10)
            r //= 10
    r = rnd()
    digits = ""
    for _ in range(11):
        digits += chr(ord("0") + r % 10)
        r //= 10
    out += "+" + digits[:4] + "-" + digits[4:] + "-"
    r = rnd()
    alphabet = "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789/"
    for _ in range(8):
        out += alphabet[r % 37]
        r //= 37
    return (out + "-").encode("ascii")


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds.  counter: [..., 4] and key: [..., 2] (or 2 numbers) of 32-bit words; returns [..., 4] uint32"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]           # 32 x 32 -> 64 bits: no wrap
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


# ------------------------------------------------------------------ modulator shared by both generators
def _dphi(tone_hz, rate):
    return int(round(4294967296.0 * tone_hz / float(rate))) & MASK32


def _bit_table(texts):
    """[n, longest] uint8 of the bits of each text, least significant bit of each byte first, and the bit counts"""
    counts = np.array([8 * len(t) for t in texts], dtype=np.int64)
    table = np.zeros((len(texts), int(counts.max())), dtype=np.uint8)
    for i, t in enumerate(texts):
        table[i, : counts[i]] = np.unpackbits(np.frombuffer(t, dtype=np.uint8), bitorder="little")
    return table, counts


def _modulate(sym_index, bits, amp, rate):
    """sym_index [T, n] (-1: silence, which also resets the phase), bits [n, nbits], amp [n] -> clean [T, n] float64, phase uint32"""
    inside = sym_index >= 0
    cols = np.broadcast_to(np.arange(sym_index.shape[1]), sym_index.shape)
    bit = bits[cols, np.where(inside, sym_index, 0)]
    step = np.where(bit == 1, np.uint64(_dphi(MARK_HZ, rate)), np.uint64(_dphi(SPACE_HZ, rate)))
    total = np.cumsum(np.where(inside, step, np.uint64(0)), axis=0, dtype=np.uint64)
    # phase since the last silent sample: the running total less its value at that sample
    at_reset = np.maximum.accumulate(np.where(inside, np.uint64(0), total), axis=0)
    phase = ((total - at_reset) & np.uint64(MASK32)).astype(np.uint32)
    angle = phase.astype(np.float32).astype(np.float64) / 2147483648.0        # the one float32 step: (float)phase
    clean = np.where(inside, amp[None, :] * np.cos(np.pi * angle), 0.0)
    return clean, phase


def _channel_draws(seed, index):
    return _Stream((seed & MASK64) ^ ((0x2545f4914f6cdd1d * ((index + 1) & MASK32)) & MASK64))


def _frac_distance(q):
    return np.abs(q - np.rint(q))


# ------------------------------------------------------------------ AWGN Monte-Carlo trials
def trials(n_trials, first_trial, n_samples, rate, seed, lo, step, n_grid, with_noise=True):
    """Expected output of same_synth_trials_device: dict of x, clean, noise [T, n] float64, g (unit normals), amp, sigma,
    sps, lead, ebn0_db, trial, payloads, n_bits per trial, sym_index [T, n] (-1 outside the burst), boundary_margin [n]."""
    fs = float(rate)
    lo, step = float(np.float32(lo)), float(np.float32(step))
    n = n_trials
    trial = [(first_trial + c) & MASK32 for c in range(n)]
    payloads = [payload(seed, t) for t in trial]
    amp, sps, lead, ebn0_db = (np.empty(n) for _ in range(4))
    for c, t in enumerate(trial):
        rnd = _channel_draws(seed, t)
        amp[c] = 2000.0 + 28000.0 * (rnd() % 65536) / 65536.0
        skew = ((rnd() % 2001) - 1000.0) * 2.5e-6
        sps[c] = fs / (BAUD * (1.0 + skew))
        lead[c] = 0.1 * fs + (rnd() % 65536) / 65536.0 * sps[c]
        ebn0_db[c] = lo + (t % n_grid) * step
    sigma = amp * np.sqrt((fs / BAUD) / (4.0 * 10.0 ** (0.1 * ebn0_db)))
    bits, n_bits = _bit_table([b"\xab" * PREAMBLE_BYTES + p for p in payloads])

    t_idx = np.arange(n_samples, dtype=np.float64)[:, None]
    q = (t_idx - lead[None, :]) / sps[None, :]
    sym = np.floor(q).astype(np.int64)
    sym_index = np.where((sym >= 0) & (sym < n_bits[None, :]), sym, -1)
    near = (q > -1.0) & (q < n_bits[None, :] + 1.0)
    boundary_margin = np.where(near, _frac_distance(q), np.inf).min(axis=0)
    clean, _ = _modulate(sym_index, bits, amp, rate)
    out = dict(clean=clean, amp=amp, sigma=sigma, sps=sps, lead=lead, ebn0_db=ebn0_db, trial=np.array(trial, dtype=np.uint64),
               payloads=payloads, n_bits=n_bits, sym_index=sym_index, boundary_margin=boundary_margin)
    if with_noise:
        g = trial_normals(trial, n_samples, seed)
        out.update(g=g, noise=sigma[None, :] * g, x=clean + sigma[None, :] * g)
    return out


def trial_normals(trial, n_samples, seed):
    """unit normals [T, n] of the trial generator: Philox4x32-10 and Box-Muller, four samples per counter"""
    n_blocks = (n_samples + 3) // 4
    block = np.arange(n_blocks, dtype=np.uint64)
    ctr = np.empty((n_blocks, len(trial), 4), dtype=np.uint64)
    ctr[..., 0] = (block & np.uint64(MASK32))[:, None]
    ctr[..., 1] = (block >> np.uint64(32))[:, None]
    ctr[..., 2] = np.asarray(trial, dtype=np.uint64)[None, :]
    ctr[..., 3] = 0x5a4d4531
    w = philox4x32_10(ctr, np.array([seed & MASK32, (seed >> 32) & MASK32], dtype=np.uint64))
    g = np.empty((n_blocks, 4, len(trial)))
    for p in range(2):
        u1 = ((w[..., 2 * p] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
        u2 = (w[..., 2 * p + 1] >> np.uint32(8)).astype(np.float64) / 16777216.0
        r = np.sqrt(-2.0 * np.log(u1))
        g[:, 2 * p, :] = r * np.cos(2.0 * np.pi * u2)
        g[:, 2 * p + 1, :] = r * np.sin(2.0 * np.pi * u2)
    return g.reshape(n_blocks * 4, len(trial))[:n_samples]


# ------------------------------------------------------------------ the multi-channel workload
def afsk(n_channels, n_samples, rate, seed, noise_sigma=0.0, integer_symbols=False, with_margin=True):
    """Expected output of same_synth_afsk_device: dict of x, clean, noise [T, n] float64, g, amp, sigma (= noise_sigma amp),
    sps, lead, payloads, sym_index [T, n] (symbol within its burst, -1 in a gap), burst [T, n] (0..5 within the cycle, -1 in
    a gap), burst_first (list per channel of the first sample of every burst that starts in the buffer), boundary_margin
    (inf without with_margin: it costs as much as all the rest)."""
    fs = float(rate)
    noise_sigma = float(np.float32(noise_sigma))
    n = n_channels
    payloads = [payload(seed, c) for c in range(n)]
    amp, sps, lead = (np.empty(n) for _ in range(3))
    for c in range(n):
        rnd = _channel_draws(seed, c)
        lead[c] = (rnd() % 1000000) * 1e-6 * fs
        amp[c] = 2000.0 + 28000.0 * (rnd() % 65536) / 65536.0
        skew = ((rnd() % 2001) - 1000.0) * 2.5e-6
        sps[c] = fs / (BAUD * (1.0 + skew))
        if integer_symbols:
            whole = int(np.floor(fs / BAUD))
            sps[c] = float(whole + (whole % 2))
    preamble = b"\xab" * PREAMBLE_BYTES
    hbits, n_hbits = _bit_table([preamble + p for p in payloads])
    n_ebits = 8 * (PREAMBLE_BYTES + len(EOM))
    bits = np.zeros((n, max(hbits.shape[1], n_ebits) * 2), dtype=np.uint8)      # header bits, then end-of-message bits
    e_off = bits.shape[1] // 2
    bits[:, : hbits.shape[1]] = hbits
    bits[:, e_off: e_off + n_ebits] = _bit_table([preamble + EOM])[0]

    # the cycle  H gap H gap H gap E gap E gap E gap2  in samples
    hdur, edur = n_hbits * sps, n_ebits * sps
    durs = np.stack([hdur, hdur, hdur, edur, edur, edur])                       # [6, n]
    gaps = np.array([fs, fs, fs, fs, fs, 2.0 * fs])[:, None]
    starts = np.concatenate([np.zeros((1, n)), np.cumsum(durs + gaps, axis=0)[:-1]])
    cycle = 3.0 * (hdur + fs) + 2.0 * (edur + fs) + edur + 2.0 * fs
    n_sym = np.stack([n_hbits] * 3 + [np.full(n, n_ebits)] * 3)

    tt = np.arange(n_samples, dtype=np.float64)[:, None] - lead[None, :]
    turns = tt / cycle[None, :]
    u = tt - cycle[None, :] * np.floor(turns)
    # the burst a sample falls into or follows: the last of the six that has started
    b_idx = np.zeros((n_samples, n), dtype=np.int64)
    for b in range(1, 6):
        b_idx += u >= starts[b][None, :]
    q = (u - np.take_along_axis(starts, b_idx, axis=0)) / sps[None, :]
    sym = np.floor(q).astype(np.int64)
    inside = (tt >= 0.0) & (sym < np.take_along_axis(n_sym, b_idx, axis=0))
    sym_index = np.where(inside, sym, -1)
    burst = np.where(inside, b_idx, -1).astype(np.int8)
    table_index = sym + np.where(b_idx >= 3, e_off, 0)
    del q, sym
    margin = np.full(n, np.inf)
    if with_margin:
        # distance, in symbols, of every sample from the lead-in's end and the wraps of the cycle, and from every symbol
        # boundary (first and last included) of every burst
        m = _frac_distance(turns) * (cycle / sps)[None, :]
        for b in range(6):
            q = (u - starts[b][None, :]) / sps[None, :]
            near = (q > -1.0) & (q < n_sym[b][None, :] + 1.0)
            m = np.minimum(m, np.where(near, _frac_distance(q), np.inf))
        margin = m.min(axis=0)
    boundary_margin = margin
    clean, _ = _modulate(np.where(sym_index >= 0, table_index, -1), bits, amp, rate)
    starts_here = (sym_index >= 0) & (np.concatenate([np.full((1, n), -1, dtype=np.int64), sym_index[:-1]]) < 0)
    burst_first = [np.flatnonzero(starts_here[:, c]) for c in range(n)]
    out = dict(clean=clean, amp=amp, sigma=noise_sigma * amp, sps=sps, lead=lead, payloads=payloads, sym_index=sym_index,
               burst=burst, burst_first=burst_first, boundary_margin=boundary_margin, x=clean)
    if noise_sigma > 0.0:
        start = np.array([((seed & MASK64) * 0x9e3779b97f4a7c15 + c * 0x632be59bd9b4e019) & MASK64 for c in range(n)],
                         dtype=np.uint64)
        r = _splitmix64_at(start[None, :], np.arange(1, n_samples + 1, dtype=np.uint64)[:, None])
        u1 = ((r >> np.uint64(40)).astype(np.float64) + 1.0) / 16777216.0
        u2 = ((r >> np.uint64(8)) & np.uint64(0xffffff)).astype(np.float64) / 16777216.0
        g = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
        out.update(g=g, noise=out["sigma"][None, :] * g, x=clean + out["sigma"][None, :] * g)
    return out


# ------------------------------------------------------------------ an ideal-timing detector
def noncoherent_fsk_bits(x, lead, sps, n_bits, rate):
    """Textbook non-coherent binary FSK detection with known timing.  x [T] or [T, n]; lead, sps, n_bits scalars or [n].
    Symbol k of a channel is the samples t with  k <= (t - lead) / sps < k + 1;  over exactly those, x is correlated with
    exp(-j 2 pi f t / fs) at the mark and at the space tone and the larger magnitude decides (mark = 1).  Returns
    [max(n_bits), n] uint8 (rows past a channel's n_bits are 0).  For orthogonal tones in white noise its bit error rate
    is exp(-Eb / 2 N0) / 2; it shares nothing with the receiver under test."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    T, n = x.shape
    lead, sps = np.broadcast_to(np.asarray(lead, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(sps, dtype=np.float64), (n,))
    n_bits = np.broadcast_to(np.asarray(n_bits, dtype=np.int64), (n,))
    k = np.minimum(np.arange(int(n_bits.max()) + 1)[:, None], n_bits[None, :]).astype(np.float64)
    edge = np.ceil(lead[None, :] + k * sps[None, :]).astype(np.int64)           # first sample of symbol k
    assert edge.min() >= 0 and edge.max() <= T, "the burst does not lie inside the buffer"
    t = np.arange(T, dtype=np.float64)
    mag = []
    for tone in (MARK_HZ, SPACE_HZ):
        z = x * np.exp(-2j * np.pi * tone / float(rate) * t)[:, None]
        acc = np.concatenate([np.zeros((1, n), dtype=np.complex128), np.cumsum(z, axis=0)])
        at = np.take_along_axis(acc, edge, axis=0)
        mag.append(np.abs(at[1:] - at[:-1]))
    decided = (mag[0] > mag[1]).astype(np.uint8)
    decided[np.arange(decided.shape[0])[:, None] >= n_bits[None, :]] = 0
    return decided


def sent_bits(ref):
    """[max(n_bits), n] uint8 of the bits a trials() result transmits (preamble and header), zero past each n_bits"""
    table, _ = _bit_table([b"\xab" * PREAMBLE_BYTES + p for p in ref["payloads"]])
    return np.ascontiguousarray(table.T)


def whole_symbols(ref, n_samples):
    """per trial, the number of leading symbols of its burst that lie wholly inside a buffer of n_samples"""
    fit = np.floor((n_samples - ref["lead"]) / ref["sps"]).astype(np.int64)
    return np.minimum(ref["n_bits"], fit)


def bit_error_z_scores(decided, ref, n_bits):
    """per grid value of ref['ebn0_db']: (Eb/N0 dB, bits, errors, z) with z = (errors - N p) / sqrt(N p (1 - p)),
    p = exp(-Eb / 2 N0) / 2; the first n_bits[c] bits of trial c count"""
    sent = sent_bits(ref)[: decided.shape[0]]
    counted = np.arange(decided.shape[0])[:, None] < n_bits[None, :]
    wrong = ((decided != sent) & counted).sum(axis=0)
    rows = []
    for db in np.unique(ref["ebn0_db"]):
        sel = ref["ebn0_db"] == db
        bits, errors = int(n_bits[sel].sum()), int(wrong[sel].sum())
        p = 0.5 * np.exp(-0.5 * 10.0 ** (0.1 * db))
        rows.append((float(db), bits, errors, float((errors - bits * p) / np.sqrt(bits * p * (1.0 - p)))))
    return rows


# ------------------------------------------------------------------ the law of unit normals
def noise_law(g, quads=True):
    """Statistics of g [T, n], per column, that unit white Gaussian noise must satisfy, each with the bound that follows
    from the sample count (5 standard errors): mean, variance, autocorrelation at lags 1, 2 and 4 and, with `quads`, the
    correlation inside the pairs (4k, 4k+1) and (4k+2, 4k+3); and the largest |g| of the whole array.
    Returns (rows, largest): rows is a list of (name, worst |value| over the columns, bound)."""
    g = np.asarray(g, dtype=np.float64)
    T = g.shape[0]
    rows = [("mean", np.abs(g.mean(axis=0)).max(), 5.0 / np.sqrt(T)),
            ("variance - 1", np.abs(g.var(axis=0) - 1.0).max(), 5.0 * np.sqrt(2.0 / T))]
    for lag in (1, 2, 4):
        rows.append((f"lag {lag}", np.abs((g[:-lag] * g[lag:]).mean(axis=0)).max(), 5.0 / np.sqrt(T - lag)))
    if quads:
        q = g[: T - T % 4].reshape(T // 4, 4, -1)
        rows.append(("pair 4k, 4k+1", np.abs((q[:, 0] * q[:, 1]).mean(axis=0)).max(), 5.0 / np.sqrt(T // 4)))
        rows.append(("pair 4k+2, 4k+3", np.abs((q[:, 2] * q[:, 3]).mean(axis=0)).max(), 5.0 / np.sqrt(T // 4)))
    return rows, float(np.abs(g).max())


LARGEST_NORMAL = (4.5, 5.8)     # sqrt(2 ln 2^24) = 5.77 is the most a 24-bit u1 in (0, 1] can give


def assert_noise_law(g, quads=True, what="noise"):
    rows, largest = noise_law(g, quads)
    for name, value, bound in rows:
        print(f"{what}: {name}: worst {value:.3e} (bound {bound:.3e})")
    print(f"{what}: largest |g| {largest:.4f}")
    for name, value, bound in rows:
        assert value < bound, (what, name, value, bound)
    assert LARGEST_NORMAL[0] < largest < LARGEST_NORMAL[1], (what, largest)


# ------------------------------------------------------------------ the shapes the GPU tests use (tests/test_synth_gpu.py)
# kept here so that tests/test_synth_reference_cpu.py can hold every one of them to the boundary margin without a GPU
def _trial_case(n_trials, first_trial, n_samples, rate, seed, lo=0.0, step=1.0, n_grid=15):
    return dict(n_trials=n_trials, first_trial=first_trial, n_samples=n_samples, rate=rate, seed=seed, lo=lo, step=step,
                n_grid=n_grid)


def _afsk_case(n_channels, n_samples, rate, seed, noise_sigma=0.0, integer_symbols=False):
    return dict(n_channels=n_channels, n_samples=n_samples, rate=rate, seed=seed, noise_sigma=noise_sigma,
                integer_symbols=integer_symbols)


TRIAL_CASES = {
    "wave_and_a_bit": _trial_case(70, 1000, 24576, 22050, 31337),         # one whole wavefront and a partial one
    "44100": _trial_case(6, 1000, 49152, 44100, 31338),
    "48000": _trial_case(6, 1000, 53504, 48000, 31339),
    "trial_number_wraps": _trial_case(70, 2 ** 32 - 35, 24576, 22050, 31340),
    "one_grid_point": _trial_case(6, 7, 24576, 22050, 31341, lo=9.0, step=1.0, n_grid=1),
    "negative_lo_fractional_step": _trial_case(16, 123456, 24576, 22050, 31342, lo=-2.5, step=0.7, n_grid=7),
    "noise_law": _trial_case(64, 0, 65536, 22050, 31343),
    "ebn0_axis": _trial_case(256, 0, 24576, 22050, 31344, lo=4.0, step=2.0, n_grid=3),
}

AFSK_CASES = {
    "one_cycle": _afsk_case(70, 11 * 22050, 22050, 424242),
    "integer_22050": _afsk_case(8, 22050 * 9 // 2, 22050, 424243, integer_symbols=True),
    "integer_44100": _afsk_case(8, 44100 * 9 // 2, 44100, 424243, integer_symbols=True),
    "integer_48000": _afsk_case(8, 48000 * 9 // 2, 48000, 424243, integer_symbols=True),
    "noisy": _afsk_case(16, 65536, 22050, 424244, noise_sigma=0.05),
}
