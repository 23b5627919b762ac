"""The stream / event protocol of the denoising loop (pipeline.drive_blocks), checked deterministically on the CPU: the driver runs on
stand-in streams and events that only write a log, and happens-before is computed over the log with one vector clock per stream.  A
missing wait is a race, and a race can pass the bit-equality tests of the GPU suite; here it is a violated ordering, every time."""
import contextlib

import pytest
import torch

from idm_vton_amd.pipeline import drive_blocks

BLOCK_COUNTS = [1, 2, 3, 4, 7]
MAIN, SIDE = "main", "side"


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(("wait_stream", self.name, other.name))

    def wait_event(self, ev):
        self.log.append(("wait_event", self.name, ev.name))


class _Event:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def record(self, stream):
        self.log.append(("record", self.name, stream.name))


def _run(nb, overlap, monkeypatch):
    """-> the log of one drive_blocks call over nb blocks: ('prepare', stream) first, then ('garment' | 'tryon', bi, p, stream) and the
    wait_stream / wait_event / record entries in host order."""
    log, current = [("prepare", MAIN)], [MAIN]

    @contextlib.contextmanager
    def on_stream(s):
        current.append(s.name)
        try:
            yield
        finally:
            current.pop()

    monkeypatch.setattr(torch.cuda, "stream", on_stream)
    blocks = [(3 * bi, 3) for bi in range(nb)]
    garment = lambda bi, p: log.append(("garment", bi, p, current[-1]))
    tryon = lambda bi, p: log.append(("tryon", bi, p, current[-1]))
    if not overlap:
        drive_blocks(blocks, garment, tryon)
    else:
        ev = lambda n: [_Event(f"{n}0", log), _Event(f"{n}1", log)]
        drive_blocks(blocks, garment, tryon, _Stream(MAIN, log), _Stream(SIDE, log), ev("ready"), ev("free"))
    assert current == [MAIN]
    return log


def _violations(log, nb):
    """Replay the log with a vector clock per stream (an operation ticks its stream's own component; record copies the stream's clock into
    the event; wait_event / wait_stream merge the event's / the other stream's clock) and list what the loop's rules (a)-(d) miss."""
    idx = {MAIN: 0, SIDE: 1}
    clock = {MAIN: [0, 0], SIDE: [0, 0]}
    events, ops = {}, {}
    merge = lambda a, b: [max(x, y) for x, y in zip(a, b)]
    for e in log:
        if e[0] == "wait_stream":
            clock[e[1]] = merge(clock[e[1]], clock[e[2]])
        elif e[0] == "wait_event":
            clock[e[1]] = merge(clock[e[1]], events.get(e[2], [0, 0]))      # an event never recorded orders nothing
        elif e[0] == "record":
            events[e[1]] = list(clock[e[2]])
        else:
            s = e[-1]
            clock[s][idx[s]] += 1
            key = e[:2] if e[0] != "prepare" else e[:1]
            assert key not in ops, f"{key} ran twice"
            ops[key] = dict(p=e[2] if e[0] != "prepare" else None, stream=s, stamp=list(clock[s]))

    def hb(x, y):
        i = idx[x["stream"]]
        return x is not y and x["stamp"][i] <= y["stamp"][i]

    bad = []
    for bi in range(nb):
        g, t = ops.get(("garment", bi)), ops.get(("tryon", bi))
        if g is None or t is None:
            bad.append(f"block {bi} did not run")
            continue
        if not hb(ops[("prepare",)], g):
            bad.append(f"(a) prepare does not happen before garment {bi}")
        if g["p"] != t["p"] or not hb(g, t):
            bad.append(f"(b) garment {bi} (set {g['p']}) does not happen before tryon {bi} (set {t['p']})")
        if bi >= 2:
            t2 = ops[("tryon", bi - 2)]
            if t2["p"] != g["p"] or not hb(t2, g):
                bad.append(f"(c) tryon {bi - 2} (set {t2['p']}) does not happen before garment {bi} overwrites set {g['p']}")
    if clock[MAIN][idx[SIDE]] < clock[SIDE][idx[SIDE]]:
        bad.append("(d) the main stream has not joined the side stream at the end")
    return bad, ops


@pytest.mark.parametrize("nb", BLOCK_COUNTS)
def test_overlap_order_respects_every_dependency(nb, monkeypatch):
    log = _run(nb, True, monkeypatch)
    bad, ops = _violations(log, nb)
    assert not bad, bad
    # placement: block 0's garment work on the main stream, every later one on the side stream, TryonNet on main, sets by block parity
    for bi in range(nb):
        assert ops[("garment", bi)]["stream"] == (MAIN if bi == 0 else SIDE) and ops[("tryon", bi)]["stream"] == MAIN
        assert ops[("garment", bi)]["p"] == ops[("tryon", bi)]["p"] == bi & 1
    assert len(ops) == 2 * nb + 1


@pytest.mark.parametrize("nb", BLOCK_COUNTS)
def test_serial_order(nb, monkeypatch):
    log = _run(nb, False, monkeypatch)
    assert log[1:] == [(kind, bi, 0, MAIN) for bi in range(nb) for kind in ("garment", "tryon")]
    assert not _violations(log, nb)[0]


def test_serial_order_ends_when_tryon_returns_true():
    ran = []
    drive_blocks([(0, 1)] * 4, lambda bi, p: ran.append(("garment", bi)), lambda bi, p: ran.append(("tryon", bi)) or bi == 1)
    assert ran == [("garment", 0), ("tryon", 0), ("garment", 1), ("tryon", 1)]


@pytest.mark.parametrize("nb", [n for n in BLOCK_COUNTS if n >= 2])
def test_checker_catches_every_missing_wait(nb, monkeypatch):
    """Not vacuous: the overlap log with any single wait_event removed, or the first wait_stream, must fail the checker.  (With one block
    nothing runs on the side stream and there is no wait to remove that matters.)"""
    log = _run(nb, True, monkeypatch)
    waits = [i for i, e in enumerate(log) if e[0] == "wait_event"]
    assert len(waits) == (nb - 1) + max(nb - 2, 0)           # ready: blocks 1 .. nb-1 on main; free: blocks 2 .. nb-1 on side
    first_ws = next(i for i, e in enumerate(log) if e[0] == "wait_stream")
    assert log[first_ws] == ("wait_stream", SIDE, MAIN)
    for i in waits + [first_ws]:
        bad, _ = _violations(log[:i] + log[i + 1:], nb)
        assert bad, f"removing {log[i]} (entry {i}) went unnoticed"
