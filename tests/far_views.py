"""Frame views whose bytes lie more than 2 and 4 GiB from their base pointer: the geometry, the decoys that make a
truncated offset visible, and the plan of byte windows that tests/test_gpu_far_views.py applies to a device buffer and
tests/test_far_views_model.py to a sparse host model.  A helper, not a test.

Everything is counted in BYTES from the start of one buffer of BUFFER_BYTES (a 16-bit view is the same bytes seen as
uint16: one buffer serves both sample types).  Every view begins
ORIGIN + phase bytes into it.  With the origin just above 2^31, an offset that loses its upper half -- taken as uint32 or
as int32 -- still lands inside the buffer: the bug sought shows as a wrong result, never as a fault.  check() asserts that
for each geometry before anything is launched.

  far frames   B = 3 dense frames FAR_PITCH = 2^31 + 2^22 bytes apart: frame 1 begins in [2^31, 2^32), frame 2 beyond
               2^32 (for uint16 its ELEMENT offset, 2^31 + 2^22, also passes 2^31).  Phases 0 and 5 bytes (2 at 16 bit):
               the second leaves nothing on a 16-byte boundary.
  far rows     B = 2, frame 1's rows between frame 0's: frame pitch stride/2 rounded up to 16.  Seven row strides per
               frame height h, from the launch guards of chess.hip / chess16.hip (seam_strides): the largest multiple of
               16 that passes each guard and the next one above, and one with (h - 1) * stride >= 2^32.  Where stride/2
               would push frame 1's last row out of the buffer (56-row frames at the seventh stride: 2^25 bytes of
               head-room against a pitch of 39 MB) the pitch is stride/4 rounded up to 16.

Decoys: for every row whose offset from the view's base is at least 2^31, every offset a reader could compute by cutting
the frame offset, the row offset or their sum to uint32 or int32 (wrong_offsets) holds the bitwise complement of the row.
Outputs: the true rows with a guard band and the same alias windows are filled with SENTINEL, and only they are read
back.

Not modelled: an ELEMENT offset of a uint16 view cut to int32.  Frame 2 of the far frames would then be sought 2^33
bytes below where it is, which no buffer of this size holds; the 16-bit entry points take pitches as 64-bit byte counts
(DESIGN.md section 8)."""
import bisect

import numpy as np

BUFFER_BYTES = 2**31 + 2**32 + 2**25
ORIGIN = 2**31 + 4096
FAR_PITCH = 2**31 + 2**22
PHASES = {1: (0, 5), 2: (0, 2)}          # bytes, by sample size
SENTINEL = 0xA5
GUARD_BAND = 64                          # sentinel bytes checked on either side of every output row

# mirrors of the library's constants (tests/test_far_views_model.py recomputes the sides from them)
OFFSET_LIMIT = 0x7fffffff                # chess.hip:906, :911, :958, :983; chess16.hip:501
V1_ROWS_AHEAD = 8                        # V1_RB of chess.hip:906 (w16), :958 (chess_pyramid_ok), :983 (chess_multi_ok)
V16_ROWS_AHEAD = 64                      # chess16.hip:501 (chess16_ok)
RESOURCE_LIMIT = 2**32                   # the clamps at 0xffffffff: chess.hip:530, :599; chess16.hip:335 (and past those at
#                                          0x7fffffff: chess.hip:546, the typed resource; chess16.hip:269, fbytes)
GUARDS = (("chess16_ok", V16_ROWS_AHEAD), ("w16/pyramid/multi", V1_ROWS_AHEAD), ("typed_ok", 0))


def _round16(v):
    return (v + 15) // 16 * 16


def guard_passes(h, stride, rows_ahead):
    """the comparison of the launch guards: (h + rows_ahead) * stride < 0x7fffffff"""
    return (h + rows_ahead) * stride < OFFSET_LIMIT


def seam_strides(h):
    """[(name, stride)]: the seven far-rows strides of frames h rows high"""
    out = []
    for name, ahead in GUARDS:
        below = (OFFSET_LIMIT - 1) // (h + ahead) // 16 * 16
        assert guard_passes(h, below, ahead) and not guard_passes(h, below + 16, ahead)
        out += [(f"{name}-", below), (f"{name}+", below + 16)]
    out.append(("past2^32", _round16(-(-RESOURCE_LIMIT // (h - 1)))))
    assert (h - 1) * out[-1][1] >= RESOURCE_LIMIT
    return out


def _u32(v):
    return v % 2**32


def _i32(v):
    v %= 2**32
    return v - 2**32 if v >= 2**31 else v


TRUNCATIONS = {"exact": lambda v: v, "uint32": _u32, "int32": _i32}


class Geometry:
    """B frames of h x w samples of `es` bytes; frame f row r begins f * pitch + r * stride bytes from the base, which
    lies `origin` bytes into the buffer"""

    def __init__(self, name, B, h, w, es, origin, pitch, stride):
        self.name, self.B, self.h, self.w, self.es = name, B, h, w, es
        self.origin, self.pitch, self.stride = origin, pitch, stride
        self.row_bytes = w * es
        assert origin % es == 0 and pitch % es == 0 and stride % es == 0 and stride >= self.row_bytes

    def offset(self, f, r):
        return f * self.pitch + r * self.stride

    def rows(self):
        return [(f, r) for f in range(self.B) for r in range(self.h)]

    def wrong_offsets(self, f, r, kinds=("uint32", "int32")):
        """where a reader or writer that cuts the frame offset, the row offset or their sum looks for row (f, r)"""
        d = self.offset(f, r)
        cuts = [TRUNCATIONS["exact"]] + [TRUNCATIONS[k] for k in kinds]
        out = {ts(tf(f * self.pitch) + tr(r * self.stride)) for tf in cuts for tr in cuts for ts in cuts}
        out.discard(d)
        return sorted(out)

    def aliases(self):
        """{(f, r): [offsets]} of the rows at least 2^31 bytes from the base"""
        return {(f, r): self.wrong_offsets(f, r) for f, r in self.rows() if self.offset(f, r) >= 2**31}

    def check(self, far=True):
        """host-side, before any launch: every true row and every alias window lies inside the buffer, and no alias
        window touches a true row (with its guard band) or another alias window"""
        true = [(self.origin + self.offset(f, r), self.row_bytes) for f, r in self.rows()]
        al = self.aliases()
        assert bool(al) == far, "a far view has rows beyond 2^31 bytes, a seam view has none"
        assert all(a for a in al.values()), "every far row has an alias"
        alias = sorted({self.origin + a for offs in al.values() for a in offs})
        for a, n in true:
            assert 0 <= a - GUARD_BAND and a + n + GUARD_BAND <= BUFFER_BYTES, (self.name, a)
        for a in alias:
            assert 0 <= a and a + self.row_bytes <= BUFFER_BYTES, (self.name, a)
        spans = sorted([(a - GUARD_BAND, a + n + GUARD_BAND, 0) for a, n in true] + [(a, a + self.row_bytes, 1) for a in alias])
        for (a0, a1, k0), (b0, b1, k1) in zip(spans, spans[1:]):
            assert a1 <= b0 or (k0 == 0 and k1 == 0), (self.name, "windows overlap", a0, a1, b0, b1)
        if self.es == 2:     # element offsets cut to uint32 are exact here (the int32 cut: see the module docstring)
            assert all(self.offset(f, r) // 2 < 2**32 for f, r in self.rows())
        return self

    def torch_view(self, buf, dtype):
        """the [B, h, w] view of the byte buffer `buf` (torch.uint8, BUFFER_BYTES long)"""
        import torch
        es = self.es
        return torch.as_strided(buf.view(dtype), (self.B, self.h, self.w), (self.pitch // es, self.stride // es, 1), self.origin // es)

    def describe(self):
        h = self.h
        sides = ", ".join(f"(h+{a})*S={(h + a) * self.stride} {'<' if guard_passes(h, self.stride, a) else '>='} 2^31-1" for _, a in GUARDS)
        return f"{self.name}: {self.w}x{h}x{self.B}, {self.es} B, stride {self.stride}, pitch {self.pitch}; {sides}; (h-1)*S={(h - 1) * self.stride}"


def far_frames(h, w, es=1, phase=0):
    """three dense frames FAR_PITCH apart"""
    assert phase in PHASES[es]
    g = Geometry(f"far-frames/phase{phase}", 3, h, w, es, ORIGIN + phase, FAR_PITCH, w * es)
    assert 2**31 <= g.offset(1, 0) < 2**32 <= g.offset(2, 0)
    return g.check()


def far_rows(h, w, which, es=1):
    """two interleaved frames at the seam stride `which` (a name or an index of seam_strides(h))"""
    names = [n for n, _ in seam_strides(h)]
    name, stride = seam_strides(h)[names.index(which) if isinstance(which, str) else which]
    room = BUFFER_BYTES - ORIGIN - GUARD_BAND
    pitch = _round16(stride // 2)
    if pitch + (h - 1) * stride + w * es > room:
        pitch = _round16(stride // 4)
    g = Geometry(f"far-rows/{name}", 2, h, w, es, ORIGIN, pitch, stride)
    assert g.row_bytes + 2 * GUARD_BAND <= pitch and pitch + g.row_bytes + 2 * GUARD_BAND <= stride
    # the six guard strides put no row 2^31 bytes out (even (h - 1/2) * stride stays below): they take the seam alone
    return g.check(far=g.offset(1, h - 1) >= 2**31)


FAR_ROWS = tuple(n for n, _ in seam_strides(56))


# ---------------------------------------------------------------------------------------------------- windows

def _as_bytes(frames):
    a = np.ascontiguousarray(frames)
    return a.view(np.uint8).reshape(a.shape[0], a.shape[1], -1)


def input_plan(g, frames, decoys=True):
    """[(buffer offset, bytes)]: the true rows of `frames` ([B, h, w] of the view's dtype) and, with `decoys`, the
    complement of every far row at each of its aliases"""
    fb = _as_bytes(frames)
    assert fb.shape == (g.B, g.h, g.row_bytes)
    plan = [(g.origin + g.offset(f, r), fb[f, r]) for f, r in g.rows()]
    if decoys:
        for (f, r), offs in g.aliases().items():
            plan += [(g.origin + a, ~fb[f, r]) for a in offs]
    return plan


def output_plan(g, expected=None):
    """[(buffer offset, bytes)]: merged windows over the true rows with their guard bands and over the alias windows,
    all SENTINEL -- or, with `expected` ([B, h, w]), what they must hold after a correct call"""
    spans = [(g.origin + g.offset(f, r) - GUARD_BAND, g.origin + g.offset(f, r) + g.row_bytes + GUARD_BAND) for f, r in g.rows()]
    spans += [(g.origin + a, g.origin + a + g.row_bytes) for offs in g.aliases().values() for a in offs]
    merged = []
    for a, b in sorted(spans):
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    plan = [(a, np.full(b - a, SENTINEL, np.uint8)) for a, b in merged]
    if expected is not None:
        eb = _as_bytes(expected)
        starts = np.array([a for a, _ in plan])
        for f, r in g.rows():
            at = g.origin + g.offset(f, r)
            k = int(np.searchsorted(starts, at, side="right")) - 1
            plan[k][1][at - plan[k][0]:at - plan[k][0] + g.row_bytes] = eb[f, r]
    return plan


def coalesce(plan):
    """the same bytes in fewer writes: entries that follow each other without a gap become one"""
    out = []
    for at, data in sorted(plan, key=lambda e: e[0]):
        if out and out[-1][0] + sum(len(d) for d in out[-1][1]) == at:
            out[-1][1].append(data)
        else:
            out.append((at, [data]))
    return [(at, np.concatenate(parts)) for at, parts in out]


def apply_plan(write, plan):
    for at, data in plan:
        write(at, data)


def plan_mismatches(read, plan):
    """the windows of `plan` that `read(offset, nbytes)` does not return as planned: [(offset, first differing byte)]"""
    bad = []
    for at, data in plan:
        got = np.asarray(read(at, len(data)))
        if not np.array_equal(got, data):
            bad.append((at, int(np.flatnonzero(got != data)[0]) if got.shape == data.shape else -1))
    return bad


class SparseBuffer:
    """host model of the buffer: only the windows ever written exist.  A read must lie inside the buffer and inside what
    was written -- device memory nobody wrote holds anything, the last case's frames included, so the model refuses."""

    def __init__(self, size=BUFFER_BYTES):
        self.size, self.windows, self.starts = size, {}, []        # windows by first byte; their first bytes, sorted

    def _touching(self, at, n):
        k = max(bisect.bisect_right(self.starts, at) - 1, 0)
        while k < len(self.starts) and self.starts[k] < at + n:
            if at < self.starts[k] + len(self.windows[self.starts[k]]):
                yield self.starts[k]
            k += 1

    def write(self, at, data):
        data = np.array(data, np.uint8)
        assert 0 <= at and at + len(data) <= self.size, ("write outside the buffer", at)
        for a in list(self._touching(at, len(data))):             # newer bytes win
            old = self.windows.pop(a)
            self.starts.remove(a)
            lo, hi = min(a, at), max(a + len(old), at + len(data))
            m = np.zeros(hi - lo, np.uint8)
            m[a - lo:a - lo + len(old)] = old
            m[at - lo:at - lo + len(data)] = data
            at, data = lo, m
        self.windows[at] = data
        bisect.insort(self.starts, at)

    def read(self, at, n):
        assert 0 <= at and at + n <= self.size, ("read outside the buffer", at)
        for a in self._touching(at, n):
            if a <= at and at + n <= a + len(self.windows[a]):
                return self.windows[a][at - a:at - a + n].copy()
        raise LookupError(f"bytes [{at}, {at + n}) were never written: a reader there sees whatever the buffer held")


def read_view(read, g, cut_frame="exact", cut_row="exact", cut_sum="exact"):
    """the frames a reader gets that cuts f * pitch, r * stride and / or their sum as named: uint8 [B, h, row_bytes]"""
    tf, tr, ts = TRUNCATIONS[cut_frame], TRUNCATIONS[cut_row], TRUNCATIONS[cut_sum]
    return np.stack([np.stack([read(g.origin + ts(tf(f * g.pitch) + tr(r * g.stride)), g.row_bytes) for r in range(g.h)]) for f in range(g.B)])


def write_view(write, g, frames, cut_frame="exact", cut_row="exact", cut_sum="exact"):
    tf, tr, ts = TRUNCATIONS[cut_frame], TRUNCATIONS[cut_row], TRUNCATIONS[cut_sum]
    fb = _as_bytes(frames)
    for f, r in g.rows():
        write(g.origin + ts(tf(f * g.pitch) + tr(r * g.stride)), fb[f, r])


CUTS = [(a, b, c) for a in TRUNCATIONS for b in TRUNCATIONS for c in TRUNCATIONS if (a, b, c) != ("exact",) * 3]
