"""tests/far_views.py against a sparse host model of its 6 GiB buffer (a dict of windows, never the bytes): what shows
that tests/test_gpu_far_views.py would fail on the bug it looks for, without building a broken kernel.

A reader or writer that cuts the frame offset, the row offset or their sum to uint32 or int32 (26 combinations) must
  - stay inside the buffer, for every geometry the helper hands out;
  - read only bytes the helper wrote (the decoys: unwritten device memory may hold the last case's frames);
  - return a frame different from the true one wherever it reads another address at all;
  - fail the output check (true rows, guard bands, alias windows) wherever it writes to another address.
The seven far-rows strides are recomputed here from the constants the helper mirrors, and must fall on the intended side
of each guard."""
import os

import numpy as np
import pytest

from tests import far_views as fv


def _geometries():
    out = [fv.far_frames(24, 40, es, ph) for es in (1, 2) for ph in fv.PHASES[es]]
    out += [fv.far_rows(56, w, n) for n in fv.FAR_ROWS for w in (64, 58)]
    out += [fv.far_rows(480, 640, n) for n in fv.FAR_ROWS]
    out += [fv.far_rows(56, 64, "past2^32", es=2)]
    return out


GEOMETRIES = _geometries()
IDS = [f"{g.name}-{g.w}x{g.h}-{g.es}B-{g.origin - fv.ORIGIN}" for g in GEOMETRIES]
FAR = [(g, i) for g, i in zip(GEOMETRIES, IDS) if g.aliases()]


def _frames(g, seed=0):
    dtype = np.uint8 if g.es == 1 else np.uint16
    return np.random.default_rng(seed).integers(0, 256 ** g.es, (g.B, g.h, g.w)).astype(dtype)


def test_the_table_has_every_geometry():
    assert len(fv.FAR_ROWS) == 7 and len(GEOMETRIES) == 4 + 14 + 7 + 1
    assert sum(1 for g in GEOMETRIES if g.aliases()) == 4 + 2 + 1 + 1        # the far frames and the strides past 2^32
    assert fv.BUFFER_BYTES == 2**31 + 2**32 + 2**25 and fv.ORIGIN == 2**31 + 4096 and fv.FAR_PITCH == 2**31 + 2**22


@pytest.mark.parametrize("h", [56, 480])
def test_seam_strides_fall_on_the_intended_side_of_each_guard(h):
    limit = 0x7fffffff                                    # chess.hip:906, :911, :958, :983 and chess16.hip:501
    ahead = {"chess16_ok": 64,                            # chess16.hip:501  (lb.h + 64) * lb.img_stride < 0x7fffffffLL
             "w16/pyramid/multi": 8,                      # chess.hip:906, :958, :983  (lb.h + V1_RB) * lb.img_stride, V1_RB = 8
             "typed_ok": 0}                               # chess.hip:911  lb.h * lb.img_stride < 0x7fffffffLL
    assert (fv.OFFSET_LIMIT, dict(fv.GUARDS)) == (limit, ahead)
    strides = dict(fv.seam_strides(h))
    assert len(strides) == 7 and all(s % 16 == 0 for s in strides.values())
    for name, a in ahead.items():
        lo, hi = strides[name + "-"], strides[name + "+"]
        assert hi == lo + 16 and (h + a) * lo < limit <= (h + a) * hi
    order = [strides[n] for n in fv.FAR_ROWS]
    assert order == sorted(order)                         # each stride passes the guards named after it and fails those before
    for k, (name, a) in enumerate(fv.GUARDS):
        for j, n in enumerate(fv.FAR_ROWS):
            assert fv.guard_passes(h, strides[n], a) == (j <= 2 * k)
    assert (h - 1) * strides["past2^32"] >= 2**32 > (h - 1) * (strides["past2^32"] - 16)      # the clamps at 0xffffffff
    assert (h - 1) * strides["typed_ok+"] + 640 < 2**31   # the six guard strides leave every row within 2^31 bytes


def test_the_table_printed_in_the_gpu_test_is_the_computed_one():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_far_views.py")) as f:
        lines = [l.split() for l in f.read().split('"""')[1].splitlines()]
    for h in (56, 480):
        for name, S in fv.seam_strides(h):
            row = next(t for t in lines if t[:3] == [name, "S", str(S)])
            for label, a in (("(h+64)S", 64), ("(h+8)S", 8), ("hS", 0)):
                k = row.index(label)
                assert row[k + 1:k + 3] == [str((h + a) * S), "<" if fv.guard_passes(h, S, a) else ">="], (h, name, label)
            assert row[row.index("(h-1)S") + 1] == str((h - 1) * S)


@pytest.mark.parametrize("g", GEOMETRIES, ids=IDS)
def test_geometry_lies_inside_the_buffer_and_its_windows_apart(g):
    g.check(far=bool(g.aliases()))
    last = g.origin + g.offset(g.B - 1, g.h - 1) + g.row_bytes
    assert g.origin >= fv.ORIGIN and last + fv.GUARD_BAND <= fv.BUFFER_BYTES
    for f, r in g.rows():
        for cut in fv.CUTS:
            at = g.origin + fv.TRUNCATIONS[cut[2]](fv.TRUNCATIONS[cut[0]](f * g.pitch) + fv.TRUNCATIONS[cut[1]](r * g.stride))
            assert 0 <= at and at + g.row_bytes <= fv.BUFFER_BYTES, (cut, f, r)


@pytest.mark.parametrize("g", [g for g, _ in FAR], ids=[i for _, i in FAR])
def test_a_truncating_reader_gets_another_frame(g):
    frames = _frames(g)
    model = fv.SparseBuffer()
    fv.apply_plan(model.write, fv.input_plan(g, frames))
    true = fv.read_view(model.read, g)
    assert np.array_equal(true, fv._as_bytes(frames))
    differing = 0
    for cut in fv.CUTS:
        moved = any(g.origin + fv.TRUNCATIONS[cut[2]](fv.TRUNCATIONS[cut[0]](f * g.pitch) + fv.TRUNCATIONS[cut[1]](r * g.stride))
                    != g.origin + g.offset(f, r) for f, r in g.rows())
        got = fv.read_view(model.read, g, *cut)             # (LookupError: it read bytes nobody wrote -- a decoy is missing)
        assert moved == (not np.array_equal(got, true)), cut
        if moved:
            for f in range(g.B):                            # a frame it misses entirely comes back as the complement
                rows = [r for r in range(g.h) if not np.array_equal(got[f, r], true[f, r])]
                assert all(np.array_equal(got[f, r], ~true[f, r]) for r in rows)
            differing += 1
    assert differing >= 8                                   # uint32 and int32, on the frame offset, the row offset or the sum
    assert not fv.plan_mismatches(model.read, fv.input_plan(g, frames))


@pytest.mark.parametrize("g", [g for g, _ in FAR], ids=[i for _, i in FAR])
def test_a_truncating_writer_fails_the_output_check(g):
    frames = _frames(g, 1)
    want = fv.output_plan(g, frames)

    def run(cut):
        model = fv.SparseBuffer()
        fv.apply_plan(model.write, fv.output_plan(g))
        fv.write_view(model.write, g, frames, *cut)
        return fv.plan_mismatches(model.read, want)
    assert run(("exact",) * 3) == []
    caught = 0
    for cut in fv.CUTS:
        moved = any(fv.TRUNCATIONS[cut[2]](fv.TRUNCATIONS[cut[0]](f * g.pitch) + fv.TRUNCATIONS[cut[1]](r * g.stride)) != g.offset(f, r)
                    for f, r in g.rows())
        bad = run(cut)
        assert moved == bool(bad), cut
        caught += moved
        if moved:                                           # both halves: a true row kept the sentinel, an alias window lost it
            hit = [(at, len(d)) for at, d in want if at in {b for b, _ in bad}]
            assert any(a <= g.origin + g.offset(f, r) < a + n for f, r in g.rows() for a, n in hit)
            assert any(a <= g.origin + x < a + n for offs in g.aliases().values() for x in offs for a, n in hit)
    assert caught >= 8


def test_a_writer_that_strays_into_a_guard_band_is_caught():
    g = fv.far_frames(24, 40)
    frames = _frames(g, 2)
    model = fv.SparseBuffer()
    fv.apply_plan(model.write, fv.output_plan(g))
    fv.write_view(model.write, g, frames)
    model.write(g.origin + g.offset(2, g.h - 1) + g.row_bytes, np.zeros(1, np.uint8))     # one byte behind the last frame
    assert len(fv.plan_mismatches(model.read, fv.output_plan(g, frames))) == 1


def test_the_model_refuses_what_the_device_cannot_promise():
    m = fv.SparseBuffer()
    m.write(100, np.arange(10, dtype=np.uint8))
    assert m.read(102, 4).tolist() == [2, 3, 4, 5]
    with pytest.raises(LookupError):
        m.read(105, 10)                                     # runs off what was written
    with pytest.raises(AssertionError):
        m.read(fv.BUFFER_BYTES - 4, 8)                      # outside the allocation: the device would fault
    with pytest.raises(AssertionError):
        m.write(-1, np.zeros(4, np.uint8))
    g = fv.far_frames(24, 40)
    fv.apply_plan(m.write, fv.input_plan(g, _frames(g), decoys=False))
    with pytest.raises(LookupError):                        # without the decoys the reader's answer is undefined: no test
        fv.read_view(m.read, g, cut_frame="uint32")
