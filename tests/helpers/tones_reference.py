"""An independent numpy restatement of the tone detector's contract (include/same_tones.h).  It reads no
library of the project: the f32 form reproduces the contract operation for operation (vectorised over all blocks of all
channels, a loop over the N positions of a block), the float64 form is a direct correlation |sum x e^{-jwn}|^2 with float64
energy, and the state machine and a generator of test messages (header bursts, silence, tone, "voice", NNNN bursts; the bursts
come from the oracle's modulator) are here too."""
import numpy as np

TONES_HZ = (853.0, 960.0, 1050.0)
ATTENTION, WAT = 1, 2
START, END = 1, 2
START_BLOCKS, END_BLOCKS = 25, 5
WAT_SHARE, ATTN_EACH_SHARE, ATTN_SUM_SHARE = 0.5, 0.15, 0.5
LIVE_SHARE = 0.015625     # 1/64, exact in f32: a block is live only when Em >= this share of E
MIN_RATE, MAX_RATE = 8000, 96000

EVENT_DTYPE = np.dtype([("channel", "<u4"), ("kind", "<u4"), ("edge", "<u4"), ("reserved", "<u4"),
                        ("sample_counter", "<u8"), ("duration", "<u8")])


def block_length(rate: int) -> int:
    if not MIN_RATE <= rate <= MAX_RATE:
        raise ValueError(f"rate {rate}")
    return rate // 25


def coefficients(rate: int) -> np.ndarray:
    """c_k = (float)(2 cos(2 pi f_k / rate)): float64 throughout, rounded once"""
    return np.array([np.float32(2.0 * np.cos(2.0 * np.pi * f / float(rate))) for f in TONES_HZ], dtype=np.float32)


def _blocks_of(x, rate):
    """x: [..., samples] -> [n, N] whole blocks, every stream cut from its first sample"""
    N = block_length(rate)
    x = np.asarray(x)
    nb = x.shape[-1] // N
    return x[..., : nb * N].reshape(x.shape[:-1] + (nb, N)), N


def blocks_f32(x, rate: int, with_energy: bool = False):
    """P_0, P_1, P_2, Em of every whole block, float32 [..., blocks, 4], in the contract's operations and order.
    x: float32 or int16 (converted exactly), [..., samples].  with_energy: (that, E float32 [..., blocks]) -- the block's
    energy with its mean, E = E + x * x over the block in order, which the live guard of qualify_f32 reads."""
    xb, N = _blocks_of(x, rate)
    shape = xb.shape[:-1]
    xb = xb.reshape(-1, N).astype(np.float32)
    c = coefficients(rate)
    n = xb.shape[0]
    s1 = [np.zeros(n, np.float32) for _ in range(3)]
    s2 = [np.zeros(n, np.float32) for _ in range(3)]
    E = np.zeros(n, np.float32)
    S = np.zeros(n, np.float32)
    for i in range(N):
        v = np.ascontiguousarray(xb[:, i])
        for k in range(3):
            t = c[k] * s1[k]
            u = t - s2[k]
            s0 = v + u
            s2[k] = s1[k]
            s1[k] = s0
        E = E + v * v
        S = S + v
    out = np.empty((n, 4), np.float32)
    for k in range(3):
        a = s1[k] * s1[k]
        b = s2[k] * s2[k]
        d = c[k] * s1[k]
        e = d * s2[k]
        out[:, k] = (a + b) - e
    inv_n = np.float32(1.0) / np.float32(N)
    out[:, 3] = E - (S * S) * inv_n
    assert out.dtype == np.float32 and E.dtype == np.float32
    if with_energy:
        return out.reshape(shape + (4,)), E.reshape(shape)
    return out.reshape(shape + (4,))


def qualify_f32(vals: np.ndarray, rate: int, E: np.ndarray):
    """(attention, wat) of blocks_f32's values and energies (of the same streams), in float32 as the contract has it"""
    N = block_length(rate)
    half_n = np.float32(N) * np.float32(0.5)
    P0, P1, P2, Em = (vals[..., k] for k in range(4))
    E = np.asarray(E)
    assert E.dtype == np.float32 and E.shape == Em.shape
    ref = Em * half_n
    live = (Em > np.float32(0.0)) & (Em >= E * np.float32(LIVE_SHARE))
    wat = live & (P2 >= np.float32(WAT_SHARE) * ref)
    attn = (live & (P0 >= np.float32(ATTN_EACH_SHARE) * ref) & (P1 >= np.float32(ATTN_EACH_SHARE) * ref)
            & ((P0 + P1) >= np.float32(ATTN_SUM_SHARE) * ref))
    return attn, wat


def ratios_f64(x, rate: int) -> np.ndarray:
    """P_k / ref of every whole block by direct correlation in float64, [..., blocks, 3]; 0 where the block has no energy
    without its mean"""
    xb, N = _blocks_of(x, rate)
    xb = xb.astype(np.float64)
    n = np.arange(N, dtype=np.float64)
    P = []
    for f in TONES_HZ:
        w = 2.0 * np.pi * f / float(rate)
        z = xb @ np.exp(-1j * w * n)
        P.append(z.real ** 2 + z.imag ** 2)
    Em = (xb * xb).sum(axis=-1) - xb.sum(axis=-1) ** 2 / N
    ref = Em * (N / 2.0)
    ok = ref > 1e-9 * np.maximum((xb * xb).sum(axis=-1), 1e-300)
    return np.stack([np.where(ok, p / np.where(ok, ref, 1.0), 0.0) for p in P], axis=-1)


def share_f64(x, rate: int) -> np.ndarray:
    """Em / E of every whole block in float64, [..., blocks]; 0 where the block has no energy"""
    xb, N = _blocks_of(x, rate)
    xb = xb.astype(np.float64)
    E = (xb * xb).sum(axis=-1)
    Em = E - xb.sum(axis=-1) ** 2 / N
    return np.where(E > 0.0, Em / np.where(E > 0.0, E, 1.0), 0.0)


def qualify_f64(r: np.ndarray, share: np.ndarray):
    """(attention, wat) of ratios_f64's ratios and share_f64's shares (of the same streams)"""
    live = (share > 0.0) & (share >= LIVE_SHARE)
    wat = live & (r[..., 2] >= WAT_SHARE)
    attn = live & (r[..., 0] >= ATTN_EACH_SHARE) & (r[..., 1] >= ATTN_EACH_SHARE) & (r[..., 0] + r[..., 1] >= ATTN_SUM_SHARE)
    return attn, wat


def clear_of_thresholds(r: np.ndarray, margin: float = 0.05) -> np.ndarray:
    """blocks whose float64 ratios lie at least `margin` from every threshold"""
    far = np.abs(r[..., 2] - WAT_SHARE) >= margin
    far &= np.abs(r[..., 0] - ATTN_EACH_SHARE) >= margin
    far &= np.abs(r[..., 1] - ATTN_EACH_SHARE) >= margin
    far &= np.abs(r[..., 0] + r[..., 1] - ATTN_SUM_SHARE) >= margin
    return far


class StateMachine:
    """one class of one channel"""

    def __init__(self):
        self.active, self.run, self.miss, self.start, self.end = 0, 0, 0, 0, 0

    def step(self, q: bool, b: int, N: int):
        """block b qualifies or not: None, (START, start, 0) or (END, end, end - start)"""
        if not self.active:
            if not q:
                self.run = 0
                return None
            if self.run == 0:
                self.start = b * N
            self.run += 1
            if self.run == START_BLOCKS:
                self.active, self.miss = 1, 0
                return (START, self.start, 0)
            return None
        if q:
            self.miss = 0
            return None
        if self.miss == 0:
            self.end = b * N
        self.miss += 1
        if self.miss == END_BLOCKS:
            self.active, self.run = 0, 0
            return (END, self.end, self.end - self.start)
        return None


class Channel:
    """both state machines of a channel over its blocks, in stream order"""

    def __init__(self, channel: int, N: int):
        self.channel, self.N, self.b = channel, N, 0
        self.sm = {ATTENTION: StateMachine(), WAT: StateMachine()}

    def reset(self):
        self.__init__(self.channel, self.N)

    def feed(self, attn, wat):
        """the next blocks' qualify bits -> events (channel, kind, edge, 0, sample_counter, duration), by block then kind"""
        out = []
        for qa, qw in zip(attn, wat):
            for kind, q in ((ATTENTION, qa), (WAT, qw)):
                e = self.sm[kind].step(bool(q), self.b, self.N)
                if e:
                    out.append((self.channel, kind, e[0], 0, e[1], e[2]))
            self.b += 1
        return out


def events_of_stream(x, rate: int, channel: int = 0):
    """the events of one whole stream (1-D), from the f32 form"""
    vals, E = blocks_f32(x, rate, True)
    attn, wat = qualify_f32(vals, rate, E)
    return Channel(channel, block_length(rate)).feed(attn, wat)


def events_bound(n: int) -> int:
    return 2 * ((n + 29) // 30 + (n + 24) // 30)


def as_records(events) -> np.ndarray:
    return np.array([tuple(e) for e in events], dtype=EVENT_DTYPE)


# ---------------------------------------------------------------------------------------------------- test messages
HEADER = b"ZCZC-WXR-TOR-039173+0030-1051700-KCLE/NWS-"
PREAMBLE = b"\xab" * 16
SCALE = 16384.0          # the bursts' amplitude: the int16 scale the receivers' tests use


def tone(kind: int, n: int, rate: float, amplitude: float = 0.5, phase: float = 0.3) -> np.ndarray:
    """n samples of the two-tone attention signal or of the 1050 Hz tone at `rate` (a float: a clock that is off)"""
    t = np.arange(n, dtype=np.float64) / rate
    if kind == WAT:
        return amplitude * np.sin(2.0 * np.pi * 1050.0 * t + phase)
    return 0.5 * amplitude * (np.sin(2.0 * np.pi * 853.0 * t + phase) + np.sin(2.0 * np.pi * 960.0 * t + 2.0 * phase))


def band_noise(n: int, rate: int, rng, lo: float = 300.0, hi: float = 3000.0, rms: float = 0.2) -> np.ndarray:
    """white noise limited to lo .. hi Hz in the frequency domain: the "voice\""""
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / rate)
    spec[(f < lo) | (f > hi)] = 0.0
    v = np.fft.irfft(spec, n)
    return v * (rms / np.sqrt(np.mean(v * v)))


def message(rate: int, kind: int, seed: int, snr_db=None, clock: float = 1.0, modulate=None, header: bytes = HEADER):
    """Three header bursts with 1-s gaps, 1 s of silence, 3 s of tone, 2 s of band-limited noise, three NNNN bursts, 1 s of
    silence, all times SCALE (bursts at amplitude 1, the tone at 0.5, the noise at 0.2 rms).  `clock`: the tone generator's clock against the receiver's (1.003: 0.3 % fast).  `snr_db`: white noise over the
    whole message at that ratio to the tone's power.  Returns (x float32, the tone's first sample, its length)."""
    if modulate is None:
        from oracle.binding import modulate_afsk
        modulate = modulate_afsk
    rng = np.random.default_rng(seed)
    gap = np.zeros(rate, np.float64)
    parts = []
    for _ in range(3):
        parts += [modulate(PREAMBLE + header, rate).astype(np.float64), gap]
    tone_at = sum(len(p) for p in parts)
    tone_len = 3 * rate
    parts.append(tone(kind, tone_len, rate * clock))
    parts.append(band_noise(2 * rate, rate, rng))
    for _ in range(3):
        parts += [modulate(PREAMBLE + b"NNNN", rate).astype(np.float64), gap]
    x = np.concatenate(parts)
    if snr_db is not None:
        p_tone = np.mean(parts[6] ** 2)
        x = x + rng.standard_normal(len(x)) * np.sqrt(p_tone / 10.0 ** (snr_db / 10.0))
    return (x * SCALE).astype(np.float32), tone_at, tone_len


# ------------------------------------------------------------------------------------- idle channels and tones on an offset
IDLE_CONSTANTS = (1, 37, 500, 12345, 30000, -30000)
IDLE_NOISY = ((37, 0.3), (500, 0.6), (500, 2), (12345, 0.6), (12345, 60), (30000, 2), (30000, 150))
TONE_DC = (0.3, 1.0, 3.0)                 # the offset of a tone of amplitude A, in A


def idle_matrix(rate: int, n_blocks: int = 30):
    """[(name, stream)]: channels on which nothing is sent -- a muted receiver behind a converter with an offset.  Integer-valued
    float64 inside int16's range, n_blocks whole blocks each, so that f32 and int16 carry the same samples."""
    N = block_length(rate)
    n = n_blocks * N
    t = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(rate + 5)
    out = [(f"constant {v}", np.full(n, float(v))) for v in IDLE_CONSTANTS]
    out += [(f"{dc} + round({s} randn)", dc + np.round(s * rng.standard_normal(n))) for dc, s in IDLE_NOISY]
    out.append(("500 + 40 sin 60 Hz", np.round(500.0 + 40.0 * np.sin(2.0 * np.pi * 60.0 * t / rate))))
    out.append(("2000 + a count per 50 samples", 2000.0 + np.floor(t / 50.0)))
    step = np.full(n, 500.0)
    step[(n_blocks // 2) * N + N // 2:] = 520.0
    out.append(("500, then 520 from the middle of a block", step))
    out.append(("zeros", np.zeros(n)))
    assert all(len(x) == n and np.all(x == np.round(x)) and np.abs(x).max() <= 32767 for _, x in out)
    return [(name, x + 0.0) for name, x in out]


def tone_on_dc_matrix(rate: int, n_blocks: int = 30):
    """[(name, kind, stream)]: the 1050 Hz tone and the two-tone at amplitude A on an offset of 0.3 A, 1 A and 3 A, scaled to a
    peak of 30 000 and rounded"""
    n = n_blocks * block_length(rate)
    out = []
    for kind, what in ((WAT, "1050 Hz"), (ATTENTION, "two-tone")):
        for d in TONE_DC:
            A = 30000.0 / (1.0 + d)
            out.append((f"{what} on {d} A", kind, np.round(tone(kind, n, rate, A) + d * A) + 0.0))
    return out
