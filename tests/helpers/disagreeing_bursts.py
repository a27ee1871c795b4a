"""Messages whose bursts disagree, as clean audio: numpy float64, no GPU, no torch.

A SAME message is sent as three header bursts and three end-of-message bursts; the receiver's transport layer votes the
header bit by bit, groups and deduplicates the bursts and delivers at deadlines (682 symbols after a burst, 5 652 after the
last).  Everywhere else in the suite the three bursts are identical.  This module builds batches in which they are not:
bursts with flipped bits, bursts that are cut, missing, late or another message's, and end-of-message bursts that are
corrupted or absent.  The audio is clean (exact silence between the bursts, no noise), so that every arithmetic decodes the
transmitted bytes and the comparisons with the oracle can be exact.

  batch()                one [T, C] float32 batch, n_per_class channels per class of CLASSES, 11.5 s
  two_message_batch()    two different messages back to back on every channel (H x 3, EOM x 3, H2 x 3): a longer batch
  deadline_starts()      from a channel's oracle events, the STARTs delivered at a deadline poll and not at a burst

Both builders sit on impairments.modulate() and impairments.header_text(); there is no second modulator.  Within a class
the flip position, the bit, the header, the amplitude (2 000 .. 30 000), the lead-in (by a fraction of a symbol) and the
silence between bursts (0.9 .. 1.2 s) vary from channel to channel.  Every draw is seeded by (seed, class); a draw that would
not give its class's outcome is redrawn here, by rule (see flip()), never patched in a test.
Float32 rounding happens once, at the end.
"""
import re

import numpy as np

from helpers import impairments as im

SECONDS = 11.5
TWO_MESSAGE_SECONDS = 18.0
LEAD_S = 0.3
EOM = b"NNNN"
# Silence in front of the first end-of-message burst: longer than the 682-symbol deadline (1.31 s), so that the deadline
# which delivers a START falls into silence, where the receiver polls its assembler, and not into the next preamble
EOM_GAP_S = 1.6
# Silence between bursts 2 and 3 of the late_third class: past the deadline, so the message is delivered before burst 3
LATE_GAP_S = 1.5
INTERBURST_SYMBOLS = 682
# The first byte of a header that a drawn error may touch.  The framer finds a burst by "ZCZC", and two bursts that differ
# inside "ZCZC-" give another error code.  Behind them, an end-of-message burst that is voted together with two header
# bursts (the assembler keeps the last three) reaches as far as its four bytes and the few the framer decodes from the
# silence behind them (frame_max_invalid + 1 = 6): where the two header bursts differ there, those bytes would decide the
# vote, and they are the one thing here that another arithmetic may decode differently.
FIRST_FLIP = 10

# class -> what its channels transmit (H: the channel's header, H2: another header)
CLASSES = (
    "unanimous",            # H, H, H
    "one_flip",             # one bit of one burst flipped (which burst varies)
    "two_flips",            # one bit flipped in each of two bursts, at different bytes
    "same_bit_twice",       # the same bit flipped in two bursts: the majority is WRONG and passes the header check
    "missing_second",       # H, -, H
    "missing_third",        # H, H, -
    "single",               # H, -, -
    "short_first",          # H[:30], H, H
    "short_third",          # H, H, H[:25]
    "high_bit_one",         # bit 7 of one byte set in one burst
    "high_bit_two",         # bit 7 of the same byte set in two bursts
    "other_third",          # H, H, H2
    "other_second",         # H, H2, H
    "three_flips_one_byte", # a different bit of the same byte flipped in each burst
    "four_bursts",          # H, H, H, H
    "two_mismatch",         # H, H^bit, -: two bursts that differ and no third to decide
    "late_third",           # H, H, long silence, H
    "eom_nnzz",             # H x 3, then NNZZ x 3: four bit errors in the prefix, more than the framer admits -- no burst
    "eom_one_bit",          # H x 3, then NNNN x 3 with one bit of byte 2 or 3 flipped, another one in each burst
    "eom_single",           # H x 3, then one NNNN
    "eom_none",             # H x 3 and nothing behind them
)
# the classes in which every header burst that is sent is sent whole (49 bytes): what the relaxed and time-parallel
# comparisons with strict mode cover
WHOLE = tuple(c for c in CLASSES if c not in ("short_first", "short_third"))
# a START must come with corrected bits (aux2, the parity errors, above zero)
CORRECTED = ("one_flip", "two_flips", "high_bit_one", "high_bit_two", "other_third", "other_second", "three_flips_one_byte")
# a burst is missing: the START comes at a deadline, not at a burst
MISSING = ("missing_second", "missing_third")

_ALLOWED = set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-/?()[]._,+ ")
_HEADER = re.compile(rb"ZCZC-[A-Za-z]{3}-[A-Za-z]{3}(-[0-9]{6})+\+[0-9]{4}-[0-9]{7}-[^\n]{3,8}-")


def is_allowed(byte):
    """the characters the reference's combiner accepts (rx/combiner.rs: letters, digits and -/?()[]._,+ and space)"""
    return byte in _ALLOWED


def is_header(text):
    """the whole of `text` is a header the reference's message parser accepts"""
    return _HEADER.fullmatch(bytes(text)) is not None


def flip(rng, header, wrong_header=False, avoid=()):
    """(position, bit) of a one-bit error in `header`: from byte FIRST_FLIP on (see there), bits 0 .. 6, and leaving a
    character the combiner accepts, so that a vote it loses still yields a byte.  wrong_header: the flipped header must still pass the header check (the
    class in which the majority is wrong).  avoid: positions already used on this channel."""
    while True:
        pos, bit = int(rng.integers(FIRST_FLIP, len(header))), int(rng.integers(0, 7))
        b = bytearray(header)
        b[pos] ^= 1 << bit
        if pos in avoid or not is_allowed(b[pos]):
            continue
        if wrong_header and not is_header(b):
            continue
        return pos, bit


def flipped(header, pos, bit):
    b = bytearray(header)
    b[pos] ^= 1 << bit
    return bytes(b)


def recipe(name, rng):
    """One channel of class `name`: (the header H, header bursts, end-of-message bursts, silence in front of the third header burst or
    None for the channel's usual gap).  A burst is a byte string, or None for a burst that is not sent (silence of a whole
    header burst's length)."""
    h, h2 = im.header_text(rng), im.header_text(rng)
    while h2 == h:
        h2 = im.header_text(rng)
    hdr, eom, late = [h, h, h], [EOM] * 3, None
    if name == "one_flip":
        pos, bit = flip(rng, h)
        hdr[int(rng.integers(0, 3))] = flipped(h, pos, bit)
    elif name == "two_flips":
        a, bit_a = flip(rng, h)
        b, bit_b = flip(rng, h, avoid=(a,))
        first = int(rng.integers(0, 3))
        hdr[first] = flipped(h, a, bit_a)
        hdr[(first + 1) % 3] = flipped(h, b, bit_b)
    elif name == "same_bit_twice":
        pos, bit = flip(rng, h, wrong_header=True)
        clean = int(rng.integers(0, 3))
        hdr = [h if i == clean else flipped(h, pos, bit) for i in range(3)]
    elif name == "missing_second":
        hdr = [h, None, h]
    elif name == "missing_third":
        hdr = [h, h, None]
    elif name == "single":
        hdr = [h, None, None]
    elif name == "short_first":
        hdr = [h[:30], h, h]
    elif name == "short_third":
        hdr = [h, h, h[:25]]
    elif name == "high_bit_one":
        pos = int(rng.integers(FIRST_FLIP, len(h)))
        hdr[int(rng.integers(0, 3))] = flipped(h, pos, 7)
    elif name == "high_bit_two":
        pos, clean = int(rng.integers(FIRST_FLIP, len(h))), int(rng.integers(0, 3))
        hdr = [h if i == clean else flipped(h, pos, 7) for i in range(3)]
    elif name == "other_third":
        hdr = [h, h, h2]
    elif name == "other_second":
        hdr = [h, h2, h]
    elif name == "three_flips_one_byte":
        while True:
            pos = int(rng.integers(FIRST_FLIP, len(h)))
            bits = rng.permutation(7)[:3]
            if all(is_allowed(flipped(h, pos, int(b))[pos]) for b in bits):
                break
        hdr = [flipped(h, pos, int(b)) for b in bits]
    elif name == "four_bursts":
        hdr, eom = [h, h, h, h], [EOM] * 2          # (a third end-of-message burst would not fit the batch's length)
    elif name == "two_mismatch":
        pos, bit = flip(rng, h)
        hdr = [h, flipped(h, pos, bit), None]
    elif name == "late_third":
        late = LATE_GAP_S
    elif name == "eom_nnzz":
        eom = [b"NNZZ"] * 3
    elif name == "eom_one_bit":
        bits = rng.permutation(5)[:3]                            # N with bit 0, 1, 2, 3 or 5 flipped: O, L, J, F, n
        eom = [flipped(EOM, int(rng.integers(2, 4)), (0, 1, 2, 3, 5)[int(b)]) for b in bits]
    elif name == "eom_single":
        eom = [EOM]
    elif name == "eom_none":
        eom = []
    return h, hdr, eom, late


def _place(x, c, rate, start_s, bursts, gap_s, amplitude, sent, late=None):
    """bursts of one channel from second start_s on, `gap_s` of silence between them; returns the second the last one ends"""
    t = start_s
    for k, data in enumerate(bursts):
        if k:
            t += late if (late is not None and k == 2) else gap_s
        length = len(data) if data is not None else 49
        if data is not None:
            x[:, c] += im.modulate(data, rate, x.shape[0], amplitude, lead=t)
            sent.append(data)
        t += 8 * (len(im.PREAMBLE) + length) / im.BAUD
    return t


def _draws(rng, n):
    amp = rng.uniform(2000.0, 30000.0, n)
    lead = LEAD_S + rng.uniform(0.0, 1.0, n) / im.BAUD          # a random fraction of a symbol
    gap = rng.uniform(0.9, 1.2, n)
    return amp, lead, gap


def batch(rate, seed, n_per_class=8, classes=CLASSES):
    """One batch of len(classes) * n_per_class channels, class k on channels k * n_per_class ...  Returns a dict:
        x          [T, C] float32 (rounded once, here)
        cls        per channel, the class name
        sent       per channel, the bytes of every burst transmitted, in order (without the preamble)
        n_header_bursts   per channel, how many of them are header bursts (the rest are end-of-message bursts)
        framed     per channel, the bursts of `sent` the framer can find (all but NNZZ)
        header     per channel, the header H the channel is about
        amplitude, rate, seed, classes, n_per_class"""
    T = int(round(rate * SECONDS))
    n = n_per_class
    C = len(classes) * n
    x = np.zeros((T, C), dtype=np.float64)
    cls, sent, n_header, header, amplitude = [], [], [], [], np.zeros(C)
    for k, name in enumerate(classes):
        # one generator per (seed, class): the draws of a class do not depend on which other classes are in the batch
        rng = np.random.default_rng([seed, 500 + CLASSES.index(name)])
        amp, lead, gap = _draws(rng, n)
        if name == "four_bursts":
            gap = 0.9 + (gap - 0.9) / 3.0                        # 0.9 .. 1.0 s: four bursts and the rest fit the batch
        for i in range(n):
            c = k * n + i
            h, hdr, eom, late = recipe(name, rng)
            s = []
            t = _place(x, c, rate, lead[i], hdr, gap[i], amp[i], s, late)
            n_header.append(len(s))
            end = _place(x, c, rate, t + EOM_GAP_S, eom, gap[i], amp[i], s) if eom else t
            assert end + 0.3 < SECONDS, (name, i, end)
            cls.append(name)
            sent.append(s)
            header.append(h)
            amplitude[c] = amp[i]
    return dict(x=x.astype(np.float32), cls=cls, sent=sent, n_header_bursts=n_header, header=header, amplitude=amplitude,
                framed=[[s for s in ch if s != b"NNZZ"] for ch in sent],
                rate=rate, seed=seed, classes=tuple(classes), n_per_class=n_per_class)


def two_message_batch(rate, seed, n_channels=8):
    """H x 3, EOM x 3, H2 x 3 on every channel: the second message begins while the first one's bursts are still in the
    assembler's history.  Odd channels carry one flipped bit in one burst of each message.  Same keys as batch();
    `header` holds (H, H2)."""
    T = int(round(rate * TWO_MESSAGE_SECONDS))
    x = np.zeros((T, n_channels), dtype=np.float64)
    rng = np.random.default_rng([seed, 599])
    amp, lead, gap = _draws(rng, n_channels)
    gap = 0.9 + (gap - 0.9) / 3.0
    sent, n_header, header = [], [], []
    for c in range(n_channels):
        h, h2 = im.header_text(rng), im.header_text(rng)
        first, second = [h, h, h], [h2, h2, h2]
        if c % 2:
            first[int(rng.integers(0, 3))] = flipped(h, *flip(rng, h))
            second[int(rng.integers(0, 3))] = flipped(h2, *flip(rng, h2))
        s = []
        t = _place(x, c, rate, lead[c], first, gap[c], amp[c], s)
        t = _place(x, c, rate, t + EOM_GAP_S, [EOM] * 3, gap[c], amp[c], s)
        end = _place(x, c, rate, t + gap[c], second, gap[c], amp[c], s)
        assert end + 1.5 < TWO_MESSAGE_SECONDS, (c, end)          # (room for the second message's deadline)
        sent.append(s)
        n_header.append(3)
        header.append((h, h2))
    return dict(x=x.astype(np.float32), cls=["two_messages"] * n_channels, sent=sent, framed=sent, n_header_bursts=n_header, header=header,
                amplitude=amp, rate=rate, seed=seed, classes=("two_messages",), n_per_class=n_channels)


def class_channels(b, name):
    k = b["classes"].index(name)
    return range(k * b["n_per_class"], (k + 1) * b["n_per_class"])


# ------------------------------------------------------------------ the oracle on a batch
def oracle_events(ob, cfg, x, threads=None, resets=None, dtype=None):
    """Per channel of x [T, C], the oracle's events -- link and transport -- as tuples
    (kind, sample_counter, symbol_count, len, aux, aux2, bytes), one full receiver per channel (ctypes releases the
    interpreter lock: the channels run on `threads` host threads).  resets: per channel, a sample at which the receiver is
    reset() (its counters then start again from 0), or None.  dtype: np.int16 feeds the samples as int16."""
    import os
    from concurrent.futures import ThreadPoolExecutor

    def tuples(evs):
        return [(int(e.kind), int(e.sample_counter), int(e.symbol_count), int(e.len), int(e.aux), int(e.aux2), e.data()) for e in evs]

    def one(c):
        col = np.ascontiguousarray(x[:, c]) if hasattr(x, "shape") else np.ascontiguousarray(x[c])
        if dtype is not None:
            col = col.astype(dtype)
        rx = ob.Receiver(cfg)
        at = None if resets is None else resets[c]
        if at is None:
            return tuples(rx.run(col))
        out = tuples(rx.run(col[:at]))
        rx.reset()
        return out + tuples(rx.run(col[at:]))

    n_ch = x.shape[1] if hasattr(x, "shape") else len(x)
    ob.lib()
    with ThreadPoolExecutor(threads or min(16, len(os.sched_getaffinity(0)))) as pool:
        return list(pool.map(one, range(n_ch)))


def messages_of(events):
    """the START / END events of one channel as (kind, sample_counter, symbol_count, text)"""
    return [(e[0], e[1], e[2], e[6]) for e in events if e[0] in (18, 19)]


def deadline_starts(events):
    """the STARTs of one channel that were delivered at a deadline poll: no Burst event at their sample"""
    bursts = {e[1] for e in events if e[0] == 3}
    return [e for e in events if e[0] == 18 and e[1] not in bursts]
