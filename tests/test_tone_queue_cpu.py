"""The tone family's host unit (sameold_amd/csrc/same_tone_queue.h: the event queue and the chunk log behind same_tones.hip)
compiled with plain g++ under ASan + UBSan and driven by tests/helpers/tone_queue_main.cpp on plain memory: both instantiations
of the log, three emulated slots whose pools are overwritten when a slot is taken again, a seeded script of calls, peeks, drops
of any size, fetches that fail and slots taken again with and without a peek in between.

The expectation is a plain model of the contract, written from include/same_tone_audio.h and not from the unit: a list of
calls, each the list of its chunks with their samples (by channel, inside a channel in slot order), concatenated in call order
and cut from the front by the drops.  What the model has to know beyond that is where a call's samples are: in its slot's pool
until a peek publishes the call or the slot is taken again, whichever comes first -- which fixes how many fetches each operation
asks for.  Every test asserts from the model alone that the script reached the cases it is there for."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

EINVAL = -1
SLOTS = 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not found")
    path = str(tmp_path_factory.mktemp("tone_queue") / "tone_queue_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "helpers", "tone_queue_main.cpp"), "-o", path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return path


_runs = {}


def run(exe, kind, seed):
    """the driver's output as {phase: [operation, ...]}; an operation is a dict with its line's numbers and the lines below it"""
    if (kind, seed) in _runs:
        return _runs[(kind, seed)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, kind, str(seed)], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.decode().split("\n") if ln]
    assert lines[-1] == ["OK"], lines[-4:]
    phases, ops = {}, None
    for w in lines[:-1]:
        if w[0] == "phase":
            ops = phases.setdefault(w[1], [])
        elif w[0] == "call":
            ops.append(dict(op="call", index=int(w[1]), slot=int(w[2]), fetches=int(w[4]), events=[], chunks=[]))
        elif w[0] == "ev":
            ops[-1]["events"].append(tuple(int(v) for v in w[1:]))
        elif w[0] == "in":
            at = w.index(":")
            c, i, *rec = (int(v) for v in w[1:at])
            ops[-1]["chunks"].append((c, i, tuple([c] + rec), [int(v) for v in w[at + 1:]]))
        elif w[0] == "peek":
            ops.append(dict(op="peek", fail_at=int(w[1]), rc=int(w[3]), n=int(w[5]), fetches=int(w[7]), out=[]))
        elif w[0] == "review":
            ops.append(dict(op="review", n=int(w[1]), out=[]))
        elif w[0] == "out":
            at = w.index(":")
            ops[-1]["out"].append((tuple(int(v) for v in w[1:at - 1]), w[at - 1], [int(v) for v in w[at + 1:]]))
        elif w[0] == "drop":
            ops.append(dict(op="drop", k=int(w[1]), rc=int(w[3])))
        elif w[0] == "poll":
            ops.append(dict(op="poll", cap=int(w[1]), n=int(w[3]), left=int(w[5]), events=[]))
        elif w[0] == "pev":
            ops[-1]["events"].append(tuple(int(v) for v in w[1:]))
        elif w[0] == "stat":
            ops.append(dict(op="stat", allocs=int(w[2]), free=int(w[4])))
        else:
            raise AssertionError(w)
    _runs[(kind, seed)] = phases
    return phases


class Model:
    """calls, chunks and drops as the contract states them"""

    def __init__(self):
        self.unpublished = []        # harvested calls that have chunks and are in no view yet, in call order
        self.in_pool = {}            # slot -> the call whose samples nobody has copied out of the slot's pool yet
        self.last_in_slot = {}       # slot -> the call that ran in it last
        self.queue = []              # the chunks of the published calls that have not been dropped: (call index, view line)
        self.events = []
        self.n_calls = 0

    def call(self, op):
        """returns the fetches that taking the slot asks for"""
        assert op["index"] == self.n_calls and op["slot"] == self.n_calls % SLOTS
        self.n_calls += 1
        waiting = self.in_pool.pop(op["slot"], None)
        if waiting is not None:
            waiting["in_pool"] = False
        chunks = [(rec, "ptr" if samples else "null", samples) for _, _, rec, samples in sorted(op["chunks"], key=lambda ch: ch[:2])]
        call = dict(index=op["index"], slot=op["slot"], chunks=chunks, in_pool=any(ch[2] for ch in chunks))
        if chunks:
            self.unpublished.append(call)
        if call["in_pool"]:
            self.in_pool[op["slot"]] = call
        self.last_in_slot[op["slot"]] = call
        self.events += sorted(op["events"], key=lambda e: e[0])          # (stable: a channel's events stay in slot order)
        return 0 if waiting is None else 1

    def peek(self, fail_at):
        """(failed, the view, fetches)"""
        fetches = 0
        while self.unpublished:
            call = self.unpublished[0]
            if call["in_pool"]:
                fetches += 1
                if fetches == fail_at:
                    return True, [], fetches
                call["in_pool"] = False
                del self.in_pool[call["slot"]]
            self.queue += [(call["index"], ch) for ch in call["chunks"]]
            self.unpublished.pop(0)
        return False, [ch for _, ch in self.queue], fetches

    def drop(self, k):
        if k > len(self.queue):
            return EINVAL
        del self.queue[:k]
        return 0


def check_script(ops):
    """holds every operation of the script phase to the model; returns the cases the script reached, as the model saw them"""
    m = Model()
    reached = set()
    view = None                      # the last successful peek's view, while no drop has come
    partial = None                   # a partial drop has come, and since then: have calls with chunks been harvested?
    short_poll = None                # a poll left events behind, and since then: has a call brought more?
    pending_fail = None              # the calls a failed peek left unpublished in front of the next one
    calls_since_peek = 0
    for op in ops:
        if op["op"] == "call":
            before = m.last_in_slot.get(op["slot"])
            fetches = m.call(op)
            assert op["fetches"] == fetches, op
            calls_since_peek += 1
            call = m.last_in_slot[op["slot"]]
            order = [ch[:2] for ch in op["chunks"]]
            if order != sorted(order) and len({c for c, _ in order}) >= 2 and any(i >= 1 for _, i in order):
                reached.add("a call whose slots are not in channel order, a channel with two chunks")
            if fetches and calls_since_peek > SLOTS:
                reached.add("a slot taken again with no peek since its call")
            if before is not None and before["chunks"] and not any(ch[2] for ch in before["chunks"]) and before in m.unpublished:
                assert fetches == 0
                reached.add("a slot whose unpublished call has only empty chunks is free at once")
            if partial is not None and call["chunks"]:
                partial = True
            if short_poll is not None and op["events"]:
                short_poll = True
        elif op["op"] == "peek":
            blocks_in_pool = sum(1 for c in m.unpublished if c["in_pool"])
            n_unpublished = len(m.unpublished)
            empties = sum(1 for c in m.unpublished if not any(ch[2] for ch in c["chunks"]))
            failed, want, fetches = m.peek(op["fail_at"])
            assert (op["rc"] != 0) == failed and op["fetches"] == fetches, op
            assert op["n"] == len(want) == len(op["out"]) and op["out"] == want, op
            calls_since_peek = 0
            if failed:
                if op["fail_at"] == 2 and blocks_in_pool == 3 == n_unpublished:
                    pending_fail = {c["index"] for c in m.unpublished} | {i for i, _ in m.queue[-1:]}
                    reached.add("a fetch that fails at the second of three unpublished blocks")
                view = None
                continue
            if pending_fail is not None:
                # nothing lost or doubled: the view holds each call's chunks in one run, the runs in call order, the three among them
                runs = [i for at, (i, _) in enumerate(m.queue) if at == 0 or m.queue[at - 1][0] != i]
                assert runs == sorted(set(runs)) and len(pending_fail) == 3 and pending_fail <= set(runs)
                reached.add("the peek behind the failed one shows all three blocks")
                pending_fail = None
            view = want
            if len({i for i, _ in m.queue}) >= 2:
                reached.add("a view of several calls")
            if any(ch[1] == "null" for ch in want):
                assert all((ch[1] == "null") == (ch[2] == []) == (ch[0][6] == 0) for ch in want)
                reached.add("an empty chunk")
            if empties:                                      # (the model counted no fetch for them, and the counts agree)
                reached.add("a call of empty chunks asks for no fetch")
            if partial:
                reached.add("what was harvested behind a partial drop follows the rest")
            partial = None
        elif op["op"] == "review":
            assert view is not None and op["n"] == len(view) and op["out"] == view, op
            if view and calls_since_peek == 3:
                reached.add("a view read again behind three calls")
        elif op["op"] == "drop":
            n = len(m.queue)
            ends_inside = 0 < op["k"] < n and m.queue[op["k"] - 1][0] == m.queue[op["k"]][0]
            rc = m.drop(op["k"])
            assert op["rc"] == rc, op
            view = None
            if op["k"] == n + 1:
                assert rc == EINVAL
                reached.add("an oversized drop")
            elif 0 < op["k"] < n:
                reached.add("a partial drop that ends inside a block" if ends_inside else "a partial drop that ends on a block's boundary")
                partial = False
        elif op["op"] == "poll":
            have = len(m.events)
            n = min(have, op["cap"])
            assert (op["n"], op["left"]) == (n, have - n) and op["events"] == m.events[:n], op
            del m.events[:n]
            if short_poll and n:
                reached.add("the rest of a short poll follows across a later call")
            short_poll = False if have > op["cap"] > 0 else None
            if short_poll is False:
                reached.add("a poll with less room than events")
    return reached


CASES = {"a call whose slots are not in channel order, a channel with two chunks", "a view of several calls", "an empty chunk",
         "a call of empty chunks asks for no fetch", "a slot whose unpublished call has only empty chunks is free at once",
         "a partial drop that ends inside a block", "a partial drop that ends on a block's boundary",
         "what was harvested behind a partial drop follows the rest", "an oversized drop", "a view read again behind three calls",
         "a slot taken again with no peek since its call", "a fetch that fails at the second of three unpublished blocks",
         "the peek behind the failed one shows all three blocks", "a poll with less room than events",
         "the rest of a short poll follows across a later call"}


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("kind", ["audio", "delivery"])
def test_views_polls_and_fetches_are_the_models(exe, kind, seed):
    ops = run(exe, kind, seed)["script"]
    reached = check_script(ops)
    assert reached == CASES, sorted(CASES - reached)
    rate = 4000 if kind == "delivery" else 0                 # (the float record's reserved word)
    recs = [ch[0] for op in ops if op["op"] == "peek" for ch in op["out"]]
    assert recs and all(r[3] == rate for r in recs) and (kind == "delivery") == any(r[5] for r in recs)


@pytest.mark.parametrize("kind", ["audio", "delivery"])
def test_the_free_list(exe, kind):
    ops = run(exe, kind, 1)["freelist"]
    check_script(ops)                                        # (the views are the model's here too)
    stats = [op for op in ops if op["op"] == "stat"]
    calls = [op for op in ops if op["op"] == "call"]
    assert len(stats) == 10 and len(calls) == 14
    # eight calls of one size, each peeked and dropped whole before the next
    assert all(sorted(len(s) for _, _, _, s in c["chunks"]) == [4] * 10 for c in calls[:8])
    assert [op["op"] for op in ops[:4]] == ["call", "peek", "drop", "stat"] and ops[2]["k"] == ops[1]["n"] == 10
    if kind == "delivery":
        assert [s["allocs"] for s in stats[:8]] == [1] * 8 and [s["free"] for s in stats[:8]] == [1] * 8
    else:                                                    # the float capture recycles nothing: a block per call
        assert [s["allocs"] for s in stats[:8]] == list(range(1, 9)) and all(s["free"] == 0 for s in stats)
    # six calls published and none dropped, then all dropped: at most kSlots + 1 blocks are kept
    assert [op["op"] for op in ops[32:]] == ["call", "peek"] * 3 + ["call"] * 3 + ["peek", "stat", "drop", "stat"]
    assert ops[-4]["n"] == ops[-2]["k"] == 3 * 5 + 3 * 15 and ops[-2]["rc"] == 0
    assert stats[-2]["free"] == 0
    assert stats[-1]["free"] == (SLOTS + 1 if kind == "delivery" else 0) and stats[-1]["allocs"] == stats[-2]["allocs"]
