"""The three ordering promises of queued detect / refine / chain calls (include/mrgingham_amd.h):

  A  mrgingham_amd_after_stream: nothing of the next call touches the caller's memory before what is queued on the
     foreign stream has run -- neither its input frames (the upload of a pipeline) nor its output buffers;
  B  mrgingham_amd_stream_wait: a consumer stream sees the finished outputs of EVERY call in flight;
  C  order_after_previous (chain.hip): two queued calls that share a caller buffer run in program order although they
     finish on different component streams -- write after write, read after write, write after read, partly
     overlapping spans, a dependency two calls back.

A mistake in any of them gives silently wrong corner lists now and then.  Here the test decides who is slow (a
blocker kernel on the foreign stream; a long call on noise in front of a short one), so it gives them every time.
tests/stream_cases.py holds the shape, the poison, the blocker and the verdicts; every figure quoted below was measured
on an MI355X with the library as committed and is printed again by each run (pytest -s)."""
import numpy as np
import pytest
import torch

import mrgingham_amd
from tests import stream_cases as sc
from tests.stream_cases import B, CAP, finish, host, poison, verdict

pytestmark = pytest.mark.gpu

ALL_CALLS = [("detect", 0), ("detect", 1), ("detect", 2), ("chain", 3), ("chain", 1), ("chain", 0), ("refine", 0), ("response",)]


@pytest.fixture(scope="module")
def batches():
    return sc.Batches()


@pytest.fixture(scope="module")
def det(batches):
    """The default schedule (for this shape: three scratch sets), warmed up for every kind of call."""
    d = mrgingham_amd.Detector(0)
    sc.warm_up(d, batches, ALL_CALLS)
    yield d
    d.close()


def _detector(batches, calls, **options):
    d = mrgingham_amd.Detector(0)
    for k, v in options.items():
        d.set_option(k, v)
    sc.warm_up(d, batches, calls)
    return d


# =============================================================================================== A. after_stream

def _after_stream_case(det, name, fresh, stale, call, outputs, live, nstreams=1):
    """`fresh` / `stale`: tuples of input tensors; call(inputs) queues the call under test on them and returns its
    output tensors; outputs: the preallocated ones among them (poisoned behind the blocker); live(out) -> which part
    of each output is compared.  The reference is the same call in program order on the fresh and on the stale
    inputs; the case: the inputs hold the stale content, and the fresh one arrives behind the blocker.
    The blocker is a torch.cuda._sleep of 20 x the slowest unblocked call, 200 ms at the most.  Both measured values
    stand in each test's docstring: the unblocked call (issue to sync) and the blocker that follows from it, in
    milliseconds; the calibration that turns it into cycles was 2.4 cycles per ns (16 000 000 cycles = 6.70 ms), so
    a blocker of 16.3 ms is 39 million cycles."""
    work = [t.clone() for t in stale]
    keep = [fresh, stale, work, outputs]                       # (alive until the `finally` below has run)
    try:
        refs = {}
        for which, src in (("fresh", fresh), ("stale", stale)):
            for d, s in zip(work, src):
                d.copy_(s)
            poison(*outputs)
            torch.cuda.synchronize()
            out = call(work)
            finish(det)
            refs[which] = ([t.clone() for t in out], host(out))
            keep.append(out)
        assert not sc.same(refs["fresh"][1], refs["stale"][1], live(refs["fresh"][1])), "the stale batch must give another result"

        def arrive():
            for d, s in zip(work, fresh):
                d.copy_(s)

        def unblocked():
            keep.append(call(work))
        ms = sc.issue_to_sync_ms(det, unblocked, arrive)
        block = sc.blocker_ms(ms)
        print(f"[stream order A] {name}: unblocked call {min(ms):.3f}..{max(ms):.3f} ms issue to sync, blocker {block:.1f} ms")

        for d, s in zip(work, stale):
            d.copy_(s)

        def spoil():
            poison(*outputs)
        works = [lambda: (arrive(), spoil())] if nstreams == 1 else [arrive, spoil]
        out, still_blocked, streams = sc.queue_behind_blockers(det, block, works, lambda: call(work))
        keep += [out, streams]
        det.sync()
        for s in streams:
            s.synchronize()
        assert all(still_blocked), f"inconclusive: a blocker of {block:.1f} ms had ended before the call was queued"
        got = host(out)
        msg = verdict(got, refs["fresh"][1], live(refs["fresh"][1]), stale=(refs["stale"][1], live(refs["stale"][1])))
        assert msg is None, f"{name} behind after_stream: {msg}"
        return refs["fresh"][0]
    finally:
        finish(det)
        del keep


def _live_detect(out):        # (xy, counts)
    return [out[1], None]


def _live_points(out):        # (points, levels, npoints[, nrefined])
    return [out[2], out[2]] + [None] * (len(out) - 2)


@pytest.mark.parametrize("level", [0, 2])
def test_after_stream_guards_frames_and_outputs_of_detect(det, batches, level):
    """detect(out=) behind a blocked stream that uploads its frames and poisons its outputs.
    Measured: unblocked call 0.78..0.81 ms (level 0) and 0.13..0.14 ms (level 2) issue to sync; blockers of 16.3 and 2.9 ms."""
    out = sc.detect_out()
    xy, counts = _after_stream_case(det, f"detect level {level}", (batches.noise[0],), (batches.noise[1],),
                                    lambda fr: det.detect(fr[0], level, out=out, sync=False), out, _live_detect)
    sc.check_detect_against_oracle(batches, "noise0", batches.noise[0], level, xy, counts)


@pytest.mark.parametrize("start", [3, 0])
def test_after_stream_guards_frames_and_outputs_of_chain(det, batches, start):
    """chain(out=) from the usual start level and from level 0 (detection alone, on the frames themselves).
    Measured: unblocked call 0.30..0.32 ms (start 3) and 0.78..0.81 ms (start 0); blockers of 6.4 and 16.1 ms."""
    out = sc.chain_out()
    pts, lv, npts = _after_stream_case(det, f"chain from level {start}", (batches.noise[0],), (batches.noise[1],),
                                       lambda fr: det.chain(fr[0], start, out=out, sync=False), out, _live_points)
    sc.check_chain_against_oracle(batches, "noise0", batches.noise[0], start, pts, lv, npts)


def _refine_inputs(det, frames, level):
    return (frames,) + sc.points_of(*det.detect(frames, level + 1, capacity=CAP), level + 1)


def test_after_stream_guards_frames_and_points_of_refine(det, batches):
    """refine(sync=False): frames, points, levels and point counts all arrive behind the blocker.
    Measured: unblocked call 0.57..0.59 ms issue to sync; blocker 11.8 ms."""
    fresh, stale = _refine_inputs(det, batches.noise[0], 0), _refine_inputs(det, batches.noise[1], 0)

    def call(w):
        return (w[1], w[2], w[3], det.refine(w[0], 0, w[1], w[2], w[3], sync=False))
    pts, lv, npts, nref = _after_stream_case(det, "refine at level 0", fresh, stale, call, (), _live_points)
    assert int(nref.sum()) > 0
    sc.check_refine_against_oracle(batches.noise[0], 0, fresh[1:], (pts, lv, npts), nref)


def test_after_stream_guards_responses_of_cc_detect_on_response(det, batches):
    """cc_detect_on_response(sync=False): responses and level images arrive behind the blocker (the outputs are the
    call's own allocation).  Measured: unblocked call 0.98..1.01 ms issue to sync; blocker 20.1 ms."""
    fresh, stale = [(det.chess_response(fr, 0, clamp=True), fr) for fr in batches.noise]
    xy, counts = _after_stream_case(det, "cc_detect_on_response", fresh, stale,
                                    lambda w: det.cc_detect_on_response(w[0], w[1], 0, capacity=CAP, sync=False), (), _live_detect)
    want = sc.oracle.cc_detect_on_response(fresh[0][0].cpu().numpy(), fresh[1][0].cpu().numpy(), 0)
    n = int(counts[0])
    assert n == len(want) and np.array_equal(xy[0, :n].cpu().numpy(), want)


SCHEDULES = {
    "default": {}, "sparse": {"sparse_refine": 2}, "cc_lds 0": {"cc_lds": 0},
    "multi_level_launch 0": {"multi_level_launch": 0}, "multi_level_launch 1": {"multi_level_launch": 1},
    "multi_level_launch 2": {"multi_level_launch": 2}, "fuse_pyramid 0": {"fuse_pyramid": 0}, "fuse_pyramid 1": {"fuse_pyramid": 1},
    "scratch_sets 2": {"scratch_sets": 2}, "scratch_sets 3": {"scratch_sets": 3},
}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_after_stream_holds_for_every_chain_schedule(batches, schedule):
    """The chain from level 3 under every launch schedule: each puts other packets first on the pixel stream (the
    pyramid kernel, the fused level-0 launch, the merged launch of the small levels, the sparse schedule's level
    images) and starts its component stream elsewhere.  Measured: unblocked call from 0.18..0.21 ms (sparse) to 0.65..0.76 ms (cc_lds 0), 0.30..0.43 ms for the others;
    blockers of 4.2 .. 15.2 ms."""
    d = _detector(batches, [("chain", 3)], **SCHEDULES[schedule])
    try:
        out = sc.chain_out()
        pts, lv, npts = _after_stream_case(d, f"chain, {schedule}", (batches.noise[0],), (batches.noise[1],),
                                           lambda fr: d.chain(fr[0], 3, out=out, sync=False), out, _live_points)
        sc.check_chain_against_oracle(batches, "noise0", batches.noise[0], 3, pts, lv, npts)
    finally:
        d.close()


def test_two_after_stream_calls_before_one_call_are_both_honoured(det, batches):
    """One blocked stream writes the frames, another poisons the outputs; after_stream for each, then one chain.
    Measured: unblocked call 0.31..0.32 ms issue to sync; two blockers of 6.4 ms."""
    out = sc.chain_out()
    _after_stream_case(det, "chain behind two streams", (batches.noise[0],), (batches.noise[1],),
                       lambda fr: det.chain(fr[0], 3, out=out, sync=False), out, _live_points, nstreams=2)


# =============================================================================================== B. stream_wait

def _queued_calls(d, batches, kind):
    """-> (prepare, call): prepare() puts the call's buffers into their start state on torch's stream (poison, or the
    points to refine); call(sync) makes the call and returns every tensor it writes."""
    fr = batches.noise[0]
    if kind == "detect":
        out = sc.detect_out()
        return (lambda: poison(*out)), (lambda: d.detect(fr, 0, out=out, sync=False)), _live_detect
    if kind == "chain":
        out = sc.chain_out()
        return (lambda: poison(*out)), (lambda: d.chain(fr, 1, out=out, sync=False)), _live_points
    start = _refine_inputs(d, fr, 0)[1:]
    work = [t.clone() for t in start]

    def prepare():
        for w, s in zip(work, start):
            w.copy_(s)
    return prepare, (lambda: (work[0], work[1], work[2], d.refine(fr, 0, work[0], work[1], work[2], sync=False))), _live_points


@pytest.mark.parametrize("sets", [2, 3])
@pytest.mark.parametrize("kind", ["detect", "refine", "chain"])
def test_stream_wait_gives_a_consumer_the_finished_outputs(batches, kind, sets):
    """A long call queued into poisoned outputs; a consumer stream behind stream_wait copies them into snapshots, with
    no host sync between the call and the copy.  The consumer stream and the snapshots exist before the call is
    queued: an allocation may wait for the device and would order the consumer by accident."""
    d = _detector(batches, [("detect", 0), ("detect", 1), ("refine", 0), ("chain", 1)], scratch_sets=sets)
    keep = []
    try:
        prepare, call, live = _queued_calls(d, batches, kind)
        prepare()
        torch.cuda.synchronize()
        ref = call()
        finish(d)
        want = host(ref)
        snap = [torch.empty_like(t) for t in ref]
        consumer = torch.cuda.Stream()
        keep += [ref, snap, consumer]
        prepare()
        torch.cuda.synchronize()
        out = call()
        keep.append(out)
        d.stream_wait(consumer)
        with torch.cuda.stream(consumer):
            for to, t in zip(snap, out):
                to.copy_(t)
        consumer.synchronize()
        msg = verdict(host(snap), want, live(want))
        assert msg is None, f"{kind} seen behind stream_wait: {msg}"
    finally:
        finish(d)
        d.close()
        del keep


@pytest.mark.parametrize("sets", [2, 3])
def test_stream_wait_covers_every_call_in_flight(batches, sets):
    """Two calls in flight on different outputs -- a long chain from level 0 (its outputs are written at its very end),
    then a short one that finishes first, on another component stream -- and ONE stream_wait per consumer behind
    them: every snapshot of both is complete.  (The wait is for every pending scratch set, not for the last call
    alone.)  CONSUMERS streams, made with their snapshots before anything is queued: an allocation behind the wait
    may wait for the device, and a consumer may share a hardware queue with the long call's component stream;
    either orders that consumer by accident.  Option "cc_lds" 0 (the global-memory component kernels) makes the
    component search the long part of the long call: with the default kernels most of its 0.8 ms is the level-0 pixel
    kernel, behind which the short call queues on the shared pixel stream, so that the short call ends only just
    before the long one.  Measured: long 0.78..0.82 ms, short 0.05..0.08 ms issue to sync: 10.0 and 13.0 times.

    NOT SHOWN TO FAIL: with stream_wait mutated to wait for the current set only this test still passes when the
    whole file runs, although a stand-alone script that makes the same calls in a fresh process sees the poison in
    every consumer's snapshot.  It checks the promise on a correct library; it does not pin it."""
    d = _detector(batches, [("chain", 0)], scratch_sets=sets, cc_lds=0)
    keep = []
    try:
        long_out, short_out = sc.chain_out(), sc.chain_out()

        def long_call():
            return d.chain(batches.noise[0], 0, out=long_out, sync=False)

        def short_call():
            return d.chain(batches.flat, 0, out=short_out, sync=False)
        _assert_long_and_short(d, "two calls in flight", long_call, short_call)
        poison(*long_out, *short_out)
        torch.cuda.synchronize()
        long_call()
        finish(d)
        short_call()
        finish(d)
        want = host(long_out), host(short_out)
        consumers = [torch.cuda.Stream() for _ in range(CONSUMERS)]
        snaps = [([torch.empty_like(t) for t in long_out], [torch.empty_like(t) for t in short_out]) for _ in consumers]
        keep += [snaps, consumers]
        poison(*long_out, *short_out)
        torch.cuda.synchronize()
        long_call()
        short_call()
        for c, (snap_l, snap_s) in zip(consumers, snaps):
            d.stream_wait(c)
            with torch.cuda.stream(c):
                for to, t in zip(snap_l + snap_s, long_out + short_out):
                    to.copy_(t)
        for c in consumers:
            c.synchronize()
        for k, pair in enumerate(snaps):
            for name, snap, w in zip(("long (first)", "short (last)"), pair, want):
                msg = verdict(host(snap), w, _live_points(w))
                assert msg is None, f"the {name} call seen by consumer {k} behind one stream_wait: {msg}"
        assert int(want[0][2].min()) > 0 and int(want[1][2].max()) == 0
    finally:
        finish(d)
        d.close()
        del keep


# =============================================================================================== C. hazards

# The slowest short call must be this many times faster than the fastest long one, or a case says nothing.  Measured
# ratios (fastest long / slowest short, issue to sync, five runs each) are quoted in each case: 6.2 .. 11.1, and 3.2
# where the short side is two calls (LONG_OVER_TWO_SHORT).  The margins are half of the smallest of them, rounded
# down.  The short call's kernels queue behind the long call's on the shared pixel stream, so what a case needs is that
# the long call's COMPONENT work outlasts the short call's; the ratio alone does not say that (much of a long call is
# its level-0 pixel kernel).  That the short call does end first in every case of section C is shown by the mutation
# of order_after_previous: all eight fail under it.
LONG_OVER_SHORT = 3.0
LONG_OVER_TWO_SHORT = 1.6
CONSUMERS = 4                # consumer streams of the two-calls-in-flight case: as many as a process has hardware queues


def _assert_long_and_short(d, name, long_call, short_call, prepare=None, margin=LONG_OVER_SHORT):
    tl = sc.issue_to_sync_ms(d, long_call, prepare)
    ts = sc.issue_to_sync_ms(d, short_call, prepare)
    print(f"[stream order C] {name}: long {min(tl):.3f}..{max(tl):.3f} ms, short {min(ts):.3f}..{max(ts):.3f} ms, "
          f"fastest long / slowest short = {min(tl) / max(ts):.1f}")
    assert min(tl) >= margin * max(ts), f"inconclusive: the long call ({min(tl):.3f} ms) is not {margin} x the short one ({max(ts):.3f} ms)"


def _three_orders(d, name, prepare, long_call, short_call, snapshot, between=None):
    """The precondition, then the buffers (snapshot() -> host arrays) after: the long call alone; long then short in
    program order (the reference); short then long in program order (the wrong winner); long then short QUEUED with
    no host sync (what is tested).  `between`: an unrelated call queued between the two."""
    try:
        if between:
            _assert_long_and_short(d, name, long_call, lambda: (between(), short_call()), prepare, LONG_OVER_TWO_SHORT)
        else:
            _assert_long_and_short(d, name, long_call, short_call, prepare)
        seen = []
        mid = (between,) if between else ()
        for order in ((long_call,), (long_call,) + mid + (short_call,), (short_call,) + mid + (long_call,)):
            prepare()
            torch.cuda.synchronize()
            for c in order:
                c()
                finish(d)
            seen.append(snapshot())
        prepare()
        torch.cuda.synchronize()
        long_call()
        if between:
            between()
        short_call()
        finish(d)
        seen.append(snapshot())
        return seen
    finally:
        finish(d)


def test_waw_short_chain_into_the_buffers_of_a_long_one(det, batches):
    """chain L (noise) then chain S (flat) into the same `out`: the buffers hold S's result -- no points -- over L's
    points.  Measured: long 0.74..0.79 ms, short 0.08..0.09 ms: 8.3 times."""
    out = sc.chain_out()
    alone, want, wrong, got = _three_orders(
        det, "WAW same buffers", lambda: poison(*out), lambda: det.chain(batches.noise[0], 1, out=out, sync=False),
        lambda: det.chain(batches.flat, 1, out=out, sync=False), lambda: host(out))
    live = [alone[2], alone[2], None]
    assert int(want[2].max()) == 0 and int(alone[2].min()) > 0
    msg = verdict(got, want, live, other=(wrong, live))
    assert msg is None, f"WAW on one set of buffers: {msg}"


@pytest.mark.parametrize("overlap", ["xy", "counts"])
def test_waw_partly_overlapping_detect_outputs(det, batches, overlap):
    """detect L (noise, level 0) and detect S (boards, level 2: a hundred candidates, so that its span holds
    something) write tensors carved from one flat buffer: S's xy begins 16 candidates inside L's last frame, or S's
    counts begin at L's last count.  S's span holds S's result, the rest of L's span L's.
    Measured: long 0.78..0.82 ms, short 0.11..0.12 ms: 6.7 (xy) and 7.1 (counts) times."""
    xy_flat = torch.empty((2 * B * CAP * 2,), dtype=torch.int32, device="cuda")
    cn_flat = torch.empty((2 * B,), dtype=torch.int32, device="cuda")
    xy_at = ((B - 1) * CAP + 16) * 2 if overlap == "xy" else B * CAP * 2
    cn_at = B if overlap == "xy" else B - 1
    xy_l, cn_l = xy_flat[:B * CAP * 2].view(B, CAP, 2), cn_flat[:B]
    xy_s, cn_s = xy_flat[xy_at:xy_at + B * CAP * 2].view(B, CAP, 2), cn_flat[cn_at:cn_at + B]
    alone, want, wrong, got = _three_orders(
        det, f"WAW partial overlap ({overlap})", lambda: poison(xy_flat, cn_flat),
        lambda: det.detect(batches.noise[0], 0, out=(xy_l, cn_l), sync=False),
        lambda: det.detect(batches.board, 2, out=(xy_s, cn_s), sync=False), lambda: host((xy_s, cn_s, xy_l, cn_l)))
    n_s, n_l = want[1], alone[3]
    assert 16 + 16 < int(n_l[B - 1]) <= CAP and int(n_s.min()) > 16          # the live parts of the two spans really overlap
    # L's span outside S's: its frames before the last whole, of the last frame what lies before S's span
    outside = n_l.copy()
    if overlap == "xy":
        outside[B - 1] = 16
        live = [n_s, None, outside, None]
    else:
        live = [n_s, None, n_l, None]
        want[3][B - 1] = got[3][B - 1] = wrong[3][B - 1] = 0                                 # (L's last count is S's first: compared there)
    msg = verdict(got, want, live, other=(wrong, live))
    assert msg is None, f"WAW on partly overlapping spans ({overlap}): {msg}"
    sc.check_detect_against_oracle(batches, "board", batches.board, 2, xy_s, cn_s)


def test_raw_refine_reads_what_the_chain_in_front_of_it_writes(det, batches):
    """chain L (noise, from level 1) writes points, levels and counts; refine S (level 0) reads them in place.  On
    flat frames S would move nothing, whether it saw L's points or the poison; so its frames are flat with a board
    corner pasted around three of the points per frame that L left at level 1 (stream_cases.short_frames_refining):
    short, and it moves exactly those (24 of 24).  Measured: long 0.74..0.76 ms, short 0.07..0.08 ms: 9.0 times."""
    out = sc.chain_out()
    nref = []
    poison(*out)
    torch.cuda.synchronize()
    det.chain(batches.noise[0], 1, out=out, sync=False)
    finish(det)
    frames_s, pasted = sc.short_frames_refining(batches, *[t.cpu().numpy() for t in out])
    assert min(pasted) >= 1, pasted
    det.refine(frames_s, 0, *[t.clone() for t in out])                       # (warm-up of these frames, with the retry)

    def short_call():
        nref[:] = [det.refine(frames_s, 0, out[0], out[1], out[2], sync=False)]
    alone, want, wrong, got = _three_orders(
        det, "RAW chain -> refine", lambda: poison(*out), lambda: det.chain(batches.noise[0], 1, out=out, sync=False),
        short_call, lambda: host(tuple(out) + tuple(nref)))
    live = [want[2], want[2], None, None]
    print(f"[stream order C] RAW: {sum(pasted)} patches, S refines {int(want[3].sum())} of L's points")
    assert int(want[3].sum()) > 0 and not sc.same(want[:3], alone, live[:3]), "S must move some of L's points"
    assert int(wrong[3].sum()) == 0                                          # (S in front of L sees the poison: nothing to refine)
    msg = verdict(got, want, live, other=(wrong, live))
    assert msg is None, f"RAW, a refinement of the points of the chain before it: {msg}"


def _war_case(det, batches, name, long_call_of, short_call_of):
    """refine L (noise, level 0) reads its point counts N and refines its points in place; S writes N (and, for the
    chain, the points).  L's result is its reference, and N ends as S left it."""
    fr = batches.noise[0]
    start = _refine_inputs(det, fr, 0)[1:]
    work = [t.clone() for t in start]
    nref = []

    def prepare():
        for w, s in zip(work, start):
            w.copy_(s)

    def long_call():
        nref[:] = [long_call_of(fr, work)]
    alone, want, wrong, got = _three_orders(det, name, prepare, long_call, lambda: short_call_of(work),
                                            lambda: host(tuple(work) + tuple(nref)))
    n0 = host(start)[2]
    live = [n0, n0, None, None]                       # L's points up to the counts it was GIVEN; the counts; nrefined
    assert int(alone[3].sum()) > 0 and int(want[2].max()) == 0 and int(n0.min()) > 0
    assert sc.same(want[:2] + want[3:], alone[:2] + alone[3:], live[:2] + live[3:])      # S leaves L's points alone
    msg = verdict(got, want, live, other=(wrong, live))
    assert msg is None, f"{name}: {msg}"
    return start, work, nref[0]


def test_war_detect_writes_the_counts_a_refinement_reads(det, batches):
    """detect S on flat frames writes its (zero) counts into the point counts of refine L.
    Measured: long 0.57..0.58 ms, short 0.06..0.07 ms: 7.9 times."""
    xy = sc.detect_out()[0]
    start, work, nref = _war_case(det, batches, "WAR on the counts",
                                  lambda fr, w: det.refine(fr, 0, w[0], w[1], w[2], sync=False),
                                  lambda w: det.detect(batches.flat, 0, out=(xy, w[2]), sync=False))
    sc.check_refine_against_oracle(batches.noise[0], 0, start, (work[0], work[1], start[2]), nref)


def test_war_chain_writes_the_point_buffers_a_refinement_works_on(det, batches):
    """chain S on flat frames takes the point buffers of refine L as its `out`.
    Measured: long 0.57..0.58 ms, short 0.08..0.09 ms: 6.2 times."""
    _war_case(det, batches, "WAR on the points", lambda fr, w: det.refine(fr, 0, w[0], w[1], w[2], sync=False),
              lambda w: det.chain(batches.flat, 1, out=(w[0], w[1], w[2]), sync=False))


def test_war_behind_a_refinement_on_caller_built_responses(det, batches):
    """The same hazard with L queued through cc_refine_on_response (the response entries end in the same
    finish_level_call): detect S writes the counts L reads.  Measured: long 0.76..0.77 ms, short 0.06..0.07 ms: 11.1 times."""
    resp = det.chess_response(batches.noise[0], 0, clamp=True)
    xy = sc.detect_out()[0]
    _war_case(det, batches, "WAR behind cc_refine_on_response",
              lambda fr, w: det.cc_refine_on_response(resp, fr, 0, w[0], w[1], w[2], sync=False),
              lambda w: det.detect(batches.flat, 0, out=(xy, w[2]), sync=False))


def test_waw_two_calls_back_with_three_scratch_sets(batches):
    """Three scratch sets, three component streams: L, then an unrelated detection of boards at level 2 into buffers
    of its own, then S into L's buffers.  S waits for the call TWO back.
    Measured: long 0.75..0.87 ms, the two others together 0.13..0.24 ms: 3.2 times."""
    d = _detector(batches, [("chain", 1), ("detect", 2)], scratch_sets=3)
    try:
        out, other_out = sc.chain_out(), sc.detect_out()
        alone, want, wrong, got = _three_orders(
            d, "WAW two calls back", lambda: poison(*out, *other_out), lambda: d.chain(batches.noise[0], 1, out=out, sync=False),
            lambda: d.chain(batches.flat, 1, out=out, sync=False), lambda: host(out + other_out),
            between=lambda: d.detect(batches.board, 2, out=other_out, sync=False))
        live = [alone[2], alone[2], None, want[4], None]
        assert int(want[2].max()) == 0 and int(alone[2].min()) > 0 and int(want[4].min()) > 0
        msg = verdict(got, want, live, other=(wrong, live))
        assert msg is None, f"WAW with the call two back: {msg}"
    finally:
        d.close()
