"""The stream ordering of queued detect / refine / chain calls: the batches, the poison, the blocker, the timing of a
call from issue to sync and the verdict on what a buffer holds, for tests/test_gpu_stream_order.py.  A helper, not a test.

What the cases stand on:

  one shape    every call takes B frames of W x H with CAP candidates / points per frame, so no queued call
               reallocates scratch (an allocation waits for the device and would order the calls by accident).
  long, short  a LONG call runs the component search of level 0 on pseudo-noise, a SHORT one on frames that are flat
               (no component at all), hold one board (a hundred) or a few patches of one.  Measured on an MI355X, issue
               to sync, B = 8: on 640 x 480 frames of noise_frame(smooth=1) a detection at level 0 takes 0.23 ms and
               a chain from level 3 0.17 ms against 0.05 .. 0.10 ms on flat frames -- no case could tell the two apart.
               On 1280 x 960 frames the noise gives, per frame, smooth=1: 1000 .. 1100 candidates at level 0 (0.62 ms),
               18 .. 32 at level 1, 0 .. 3 at level 3; smooth=0: 2100 .. 2240 (0.78 .. 0.83 ms), 150 .. 177, 6 .. 14.
               Flat frames of that size: 0.06 .. 0.07 ms (detect, refine), 0.11 .. 0.13 ms (chain from level 3).  So
               the frames are 1280 x 960 of unsmoothed noise, and a long chain starts at level 0 or 1: from level 3
               it has a dozen points to follow and is as short as any (0.31 ms).
               The test decides who is slow, so a missing wait shows every time, not now and then.
  poison       output buffers start as POISON bytes.  Doubles are compared as int64: the poison is no number that
               equals itself in every format, its bytes are.
  lifetime     whatever a queued call may touch stays referenced until finish() has run, in a `finally`: a wait that
               is missing gives wrong bytes, never an access to freed memory.
  expected     the same calls with finish() between them (program order), one frame of which the tests hold against
               the oracle.
"""
import time

import numpy as np
import torch

from mrgingham_amd import synth
from oracle import oracle

W, H, B = 1280, 960, 8
CAP = 4096                   # candidates (detect) and points (refine, chain) per frame: the noise frames give up to 2239
POISON = 0x5A
PATCH = 16                   # half the side of the board patch short_frames_refining() pastes around a point


class Batches:
    """The frames of every case, on the device: two noise batches (the long calls; one is the other's stale
    content), a flat one and one of boards (the short calls)."""

    def __init__(self):
        self.noise = [torch.stack([synth.noise_frame(W, H, 8 * k + f, smooth=0, device="cuda") for f in range(B)]).contiguous()
                      for k in range(2)]
        self.flat = torch.full((B, H, W), 128, dtype=torch.uint8, device="cuda")
        self.board = synth.board_batch(B, W, H, 10, 0, device="cuda").contiguous()
        torch.cuda.synchronize()
        self._oracle = {}

    def oracle_once(self, key, compute):
        """The oracle's answer for one frame, computed once per module run."""
        if key not in self._oracle:
            self._oracle[key] = compute()
        return self._oracle[key]


def detect_out(n=B):
    return (torch.empty((n, CAP, 2), dtype=torch.int32, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda"))


def chain_out():
    return (torch.empty((B, CAP, 2), dtype=torch.float64, device="cuda"), torch.empty((B, CAP), dtype=torch.int8, device="cuda"),
            torch.empty((B,), dtype=torch.int32, device="cuda"))


def poison(*tensors):
    """POISON into every byte, on torch's current stream."""
    for t in tensors:
        t.view(torch.uint8).fill_(POISON)


def points_of(xy, counts, level):
    """The candidates of a detection at `level` as the points a refinement at level - 1 takes."""
    return ((xy.to(torch.float64) / 1000.0).contiguous(), torch.full(xy.shape[:2], level, dtype=torch.int8, device=xy.device),
            counts.clone())


def short_frames_refining(batches, pts, lv, npts, per_frame=3):
    """Frames on which a refinement at level 0 is short and still moves some of the given points (host arrays: pts
    float64 [B,P,2], lv [B,P], npts [B]): flat ones with a piece of a board frame, 2 * PATCH on a side and one X-corner
    in its middle, pasted around up to `per_frame` of the points that stand at level 1, away from the border and from
    each other.  A refinement on flat frames moves nothing, so nobody could tell which points it saw.
    -> (frames uint8 [B,H,W] on the device, the patches per frame)."""
    board = batches.board[0].cpu().numpy()
    corners = oracle.find_corners(board, 0).astype(np.float64) / 1000.0
    assert len(corners) == 100
    spacing = [np.sort(np.abs(corners - c).max(axis=1))[1] for c in corners]
    cx, cy = np.round(corners[int(np.argmax(spacing))]).astype(int)           # the corner farthest from its neighbours
    assert max(spacing) > 2 * PATCH and PATCH <= cx < W - PATCH and PATCH <= cy < H - PATCH
    patch = board[cy - PATCH:cy + PATCH, cx - PATCH:cx + PATCH]
    frames = np.full((B, H, W), 128, dtype=np.uint8)
    pasted = []
    for f in range(B):
        taken = []
        for i in range(int(npts[f])):
            x, y = int(np.round(pts[f, i, 0])), int(np.round(pts[f, i, 1]))
            if lv[f, i] != 1 or not (3 * PATCH <= x < W - 3 * PATCH and 3 * PATCH <= y < H - 3 * PATCH):
                continue
            if any(max(abs(x - u), abs(y - v)) < 3 * PATCH for u, v in taken):
                continue
            frames[f, y - PATCH:y + PATCH, x - PATCH:x + PATCH] = patch
            taken.append((x, y))
            if len(taken) == per_frame:
                break
        pasted.append(len(taken))
    return torch.from_numpy(frames).cuda(), pasted


def finish(det):
    det.sync()
    torch.cuda.synchronize()


def warm_up(det, batches, calls):
    """Each kind of call once, synchronously and with the capacity retry, on every batch: the component tables have
    grown to what the noisiest frame asks for, and no queued call ends in ERR_CAPACITY or allocates.
    `calls`: ("detect", level), ("chain", start), ("refine", level), ("response",)."""
    for fr in batches.noise + [batches.board, batches.flat]:
        for c in calls:
            if c[0] == "detect":
                det.detect(fr, c[1], capacity=CAP)
            elif c[0] == "chain":
                det.chain(fr, c[1], CAP)
            elif c[0] == "refine":
                p, l, n = points_of(*det.detect(fr, c[1] + 1, capacity=CAP), c[1] + 1)
                det.refine(fr, c[1], p, l, n)
            else:
                resp = det.chess_response(fr, 0, clamp=True)
                p, l, n = points_of(*det.cc_detect_on_response(resp, fr, 0, capacity=CAP), 1)
                det.cc_refine_on_response(resp, fr, 0, p, l, n)
    finish(det)


def issue_to_sync_ms(det, call, prepare=None, runs=5):
    """Milliseconds from the issue of call() to the end of det.sync(), `runs` times; prepare() (and a wait for it)
    comes before each and is not timed."""
    out = []
    for _ in range(runs):
        if prepare:
            prepare()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        det.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return out


_ms_per_cycle = None


def sleep_cycles(ms):
    """The argument of torch.cuda._sleep that keeps a stream busy for `ms` milliseconds: calibrated once, with two
    events around one _sleep long enough (>= 2 ms) for the launch not to count.  Measured on an MI355X: 16 000 000
    cycles = 6.70 ms, 2.4 cycles per ns; the blockers of 2.9 .. 20.1 ms of the tests are 7 .. 48 million cycles."""
    global _ms_per_cycle
    if _ms_per_cycle is None:
        cycles = 1_000_000
        torch.cuda._sleep(cycles)                      # (the kernel is loaded)
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            took = e0.elapsed_time(e1)
            if took >= 2.0 or cycles >= 1 << 40:
                break
            cycles *= 4
        assert took >= 2.0, f"torch.cuda._sleep({cycles}) took {took} ms: no blocker can be built from it"
        _ms_per_cycle = took / cycles
        print(f"[stream order] torch.cuda._sleep: {1e-6 / _ms_per_cycle:.1f} cycles per ns ({cycles} cycles = {took:.2f} ms)")
    return max(1, int(ms / _ms_per_cycle))


BLOCKER_FACTOR, BLOCKER_MAX_MS = 20.0, 200.0


def blocker_ms(call_ms):
    """How long the blocker of an after_stream case runs: BLOCKER_FACTOR x the slowest unblocked call (issue to
    sync), BLOCKER_MAX_MS at the most.  Generous, because the case must never fail on a correct library: the call is
    issued and would have finished many times over while the blocker still runs."""
    return min(BLOCKER_FACTOR * max(call_ms), BLOCKER_MAX_MS)


def queue_behind_blockers(det, ms, works, call):
    """One side stream per entry of `works`: a blocker of `ms` milliseconds, an event behind it, then work() -- what
    writes the call's inputs and poisons its outputs -- and det.after_stream(that stream).  Then call() queues the
    call under test.  -> (what call() returned, per stream whether its blocker still ran when the call had been
    queued, the streams).  The caller finishes the detector and the streams."""
    cycles = sleep_cycles(ms)
    streams = [torch.cuda.Stream() for _ in works]
    events = []
    torch.cuda.synchronize()
    for s, work in zip(streams, works):
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            e = torch.cuda.Event()
            e.record()
            events.append(e)
            work()
        det.after_stream(s)
    out = call()
    still_blocked = [not e.query() for e in events]
    return out, still_blocked, streams


# ---------------------------------------------------------------------------------------------- what a buffer holds

def host(tensors):
    """Device tensors as numpy arrays, doubles as their int64 bit patterns."""
    out = []
    for t in tensors:
        a = t.detach().cpu().numpy()
        out.append(a.view(np.int64) if a.dtype == np.float64 else a)
    return tuple(out)


def _part(a, n):
    """What of array `a` is compared: all of it (n is None), or the first n[f] rows of frame f."""
    if n is None:
        return a.reshape(-1)
    n = np.clip(np.asarray(n, dtype=np.int64), 0, a.shape[1])
    return a[np.arange(a.shape[1])[None, :] < n[:, None]]


def same(got, want, live):
    return all(np.array_equal(_part(g, n), _part(w, n)) for g, w, n in zip(got, want, live))


def has_poison(got, live):
    return any(bool((_part(g, n) == int.from_bytes(bytes([POISON]) * g.dtype.itemsize, "little")).any()) for g, n in zip(got, live))


def verdict(got, want, live, stale=None, other=None):
    """None when `got` (a tuple of host() arrays) is `want` -- array k whole where live[k] is None, else the first
    live[k][f] rows of frame f -- and otherwise what was seen instead.  `stale`, `other`: (arrays, live) of the result
    on the stale inputs and of the other call's result (the two calls in the wrong order)."""
    if same(got, want, live):
        return None
    seen = []
    if stale is not None and same(got, stale[0], stale[1]):
        seen.append("equals the stale reference: the call read its inputs early")
    if has_poison(got, live):
        seen.append("contains poison: written early and overwritten, or the snapshot was taken early")
    if other is not None and same(got, other[0], other[1]):
        seen.append("equals the other call's result: the wrong call won")
    differ = [k for k, (g, w, n) in enumerate(zip(got, want, live)) if not np.array_equal(_part(g, n), _part(w, n))]
    return f"tensors {differ} differ from the reference in program order; " + ("; ".join(seen) if seen else "neither stale, poison nor the other call's")


# ---------------------------------------------------------------------------------------------- the oracle, one frame

def check_detect_against_oracle(batches, name, frames, level, xy, counts, f=0):
    want = batches.oracle_once(("detect", name, level, f), lambda: oracle.find_corners(frames[f].cpu().numpy(), level))
    n = int(counts[f])
    assert n == len(want) <= CAP and np.array_equal(xy[f, :n].cpu().numpy(), want), (name, level)


def check_chain_against_oracle(batches, name, frames, start, pts, lv, npts, f=0):
    wp, wl = batches.oracle_once(("chain", name, start, f), lambda: oracle.chain(frames[f].cpu().numpy(), start))
    n = int(npts[f])
    assert n == len(wp) <= CAP and np.array_equal(pts[f, :n].cpu().numpy(), wp) and np.array_equal(lv[f, :n].cpu().numpy(), wl), (name, start)


def check_refine_against_oracle(frames, level, before, after, nref, f=0):
    """before / after: (points, levels, npoints) of the refinement at `level` on `frames`."""
    n = int(before[2][f])
    wp, wl, wn = oracle.refine_corners(before[0][f, :n].cpu().numpy(), before[1][f, :n].cpu().numpy(), frames[f].cpu().numpy(), level)
    assert np.array_equal(after[0][f, :n].cpu().numpy(), wp) and np.array_equal(after[1][f, :n].cpu().numpy(), wl) and int(nref[f]) == wn
