// The grid finder as phases over one candidate list: the text that grid_find.hip runs with one workgroup per list and
// grid_model.cpp runs serially on the host (mrgingham_amd_find_grids_host), phase loop by phase loop.  It restates
// grid.cpp under its canonical_start ring rule, and makes DECISIONS only: the product is gridn^2 candidate indices in board
// order, and whoever wants corners divides xy[index] by 1000.0 (find_grid.cc:353-354).  See include/mrgingham_amd.h for the
// contract of the entry points and DESIGN.md section 4.25 for the phases, the decline rule and the guard band.
//
// A phase is "for every item i: f(i)", written as `for (int i = x.lane(); i < n; i += x.lanes())`, with x.barrier()
// between phases.  The executor X is the only thing that differs between the two sides: 256 lanes and a workgroup
// barrier on the device, one lane and no barrier on the host.  No phase reads what another item of the same phase
// writes, a list's answer is a function of its input alone, and every arithmetic operation is an IEEE one that both
// sides round alike (integers, exact double products and sums, correctly rounded sqrt and division, single-precision
// segments_cross without contraction): the two sides agree list for list, statuses and decline reasons included.
//
// The device never gives an answer that differs from the host finder's.  Where it cannot be sure, it declines:
//   -1 count: more candidates than kGfMaxSites, or count > capacity, or count < 0
//   -2 a neighbour ring that is not mutual (site v lists b, b does not list v): nothing here resolves it
//   -3 a comparison of the sequence walk within the guard band of its threshold (the host's hypot and this file's
//      sqrt may differ by an ulp; a decision closer to its threshold than the band is the host's)
//   -4 a table is full (ring, adjacency, sequences, outer edges, cycles)
//   -5 a coordinate with |x| or |y| >= 2^24
// Every loop below runs over a range that is bounded by one of the table sizes or by gridn: garbage input ends as a
// status, never as a longer loop.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define MRG_GF_HD __host__ __device__ inline
#else
#define MRG_GF_HD inline
#endif

// (segments_cross and the walk's comparisons: no fused multiply-add on either side.  hipcc contracts device code unless
// told otherwise; g++ knows no such pragma and is given -ffp-contract=off, which on x86-64 without -march is its way anyhow)
#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace mrg {

constexpr int kGfLanes = 256;
constexpr int kGfMaxSites = 512;                  // candidates per list the device takes
constexpr int kGfMinGridn = 2, kGfMaxGridn = 16;
constexpr int kGfRingCap = 64;                    // neighbours per site
constexpr int kGfMaxAdj = 12 * kGfMaxSites;       // adjacency entries: at most 3 N - 6 Voronoi edges, both directions, each with an in-between site
constexpr int kGfMaxSeq = 4096;                   // sequence candidates
constexpr int kGfMaxOuter = 2048;                 // outer-edge candidates
constexpr int kGfMaxCycles = 256;                 // 4-cycles of outer edges
constexpr int kGfCoordLimit = 1 << 24;
constexpr int kGfGuardBitsDefault = 33, kGfGuardBitsMin = 8, kGfGuardBitsMax = 45;

enum : int {
    kGfRunning = 2,  // (never reported)
    kGfFound = 1,
    kGfNone = 0,
    kGfDeclineCount = -1,
    kGfDeclineRing = -2,
    kGfDeclineGuard = -3,
    kGfDeclineTable = -4,
    kGfDeclineCoord = -5,
};

constexpr uint16_t kGfNoSite = 0xFFFF;
constexpr uint8_t kGfDup = 1;

// thresholds, find_grid.cc:204-207
constexpr double kGfSpacingCos = 0.984, kGfRatioMin = 0.7, kGfRatioMax = 1.4, kGfRatioDev = 0.35;

// What a list's workgroup keeps close (LDS on the device): 37 KB
struct GfNear {
    int32_t sx[kGfMaxSites], sy[kGfMaxSites];  // the sites in cell order: sorted by (x, y, candidate index)
    uint16_t orig[kGfMaxSites];                // their candidate indices
    uint16_t deg[kGfMaxSites];                 // ring lengths
    uint8_t flags[kGfMaxSites];                // kGfDup: an exact duplicate of the site before it (no cell of its own)
    uint8_t hull[kGfMaxSites];                 // the site lies on the hull: its ring has a gap (written by the site's own item of phase 2)
    uint16_t adj_off[kGfMaxSites + 1];         // site -> its adjacency entries
    uint16_t seq_off[kGfMaxSites + 1];         // site -> the sequences that start there (they are found in site order)
    uint16_t out_off[kGfMaxSites + 1];         // site -> the outer edges that start there
    union { uint16_t seq_c0[kGfMaxSeq]; int32_t rx[kGfMaxSites]; };  // a sequence's first site; in phase 1, the raw x
    union { uint16_t seq_cl[kGfMaxSeq]; int32_t ry[kGfMaxSites]; };  // a sequence's last site; in phase 1, the raw y
    uint16_t outer[kGfMaxOuter];               // outer-edge candidates: indices into the sequences
    uint8_t used[kGfMaxOuter];
    uint16_t cyc[kGfMaxCycles][4];             // 4-cycles: positions in `outer`
    int32_t tmp[kGfLanes];                     // partial sums of the compaction; the tail's rows
    int32_t n, gridn, status, nadj, nseq, nouter;
};
static_assert(sizeof(GfNear) <= 40 * 1024, "one LDS slot beside the pixel kernels");
static_assert(sizeof(int32_t) * kGfMaxSites <= sizeof(uint16_t) * kGfMaxSeq, "the raw coordinates take no room of their own");
static_assert(kGfMaxAdj < 0xFFFF && kGfMaxSeq < 0xFFFF && kGfMaxSites < 0x7FFF, "16-bit tables");

// What goes to memory (a slot of context scratch on the device): the rings and the adjacency lists
struct GfFar {
    uint16_t ring[kGfMaxSites * kGfRingCap];  // per site, counter-clockwise; a hull site's begins behind its gap
    uint16_t a_site[kGfMaxAdj];               // adjacency entries in the visiting order of for_each_adjacent ...
    uint16_t a_src[kGfMaxAdj];                // ... the site they belong to
    int32_t a_dx[kGfMaxAdj], a_dy[kGfMaxAdj];
    double a_len[kGfMaxAdj];
    uint16_t a_clast[kGfMaxAdj];              // where the walk that starts with the entry ends, or kGfNoSite
    uint16_t seq_e[kGfMaxSeq];                // a sequence's first adjacency entry
};

MRG_GF_HD long long gf_orient(const GfNear& s, int a, int b, int c) {
    return (long long)(s.sx[b] - s.sx[a]) * (long long)(s.sy[c] - s.sy[a]) - (long long)(s.sy[b] - s.sy[a]) * (long long)(s.sx[c] - s.sx[a]);
}

// > 0 when d lies strictly inside the circumcircle of the counter-clockwise triangle a, b, c; exact.  Differences are
// below 2^25: squared lengths and 2x2 minors are exact doubles, and a determinant further from 0 than the rounding of
// three products and two sums can move it has its sign (grid.cpp: incircle)
MRG_GF_HD int gf_incircle(const GfNear& s, int a, int b, int c, int d) {
    const long long ax = (long long)s.sx[a] - s.sx[d], ay = (long long)s.sy[a] - s.sy[d];
    const long long bx = (long long)s.sx[b] - s.sx[d], by = (long long)s.sy[b] - s.sy[d];
    const long long cx = (long long)s.sx[c] - s.sx[d], cy = (long long)s.sy[c] - s.sy[d];
    const long long a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
    const long long ma = bx * cy - by * cx, mb = ax * cy - ay * cx, mc = ax * by - ay * bx;
    const double t1 = (double)a2 * (double)ma, t2 = (double)b2 * (double)mb, t3 = (double)c2 * (double)mc;
    const double det = t1 - t2 + t3;
    const double bound = 1e-15 * (fabs(t1) + fabs(t2) + fabs(t3));
    if (det > bound || det < -bound) return det > 0 ? 1 : -1;
    const __int128 e = (__int128)a2 * ma - (__int128)b2 * mb + (__int128)c2 * mc;
    return e > 0 ? 1 : (e < 0 ? -1 : 0);
}

// The Voronoi neighbour of p that follows its neighbour q counter-clockwise (dir > 0) or clockwise (dir < 0): the site
// strictly on that side of p -> q whose circle through p and q holds no other.  Sites that share the circle have no
// neighbourhood across it (grid.cpp:297-311): of those, the one next to p on the circle is the neighbour.  -1: no site
// on that side, p lies on the hull and q is its last neighbour this way.
MRG_GF_HD int gf_next_neighbour(const GfNear& s, int p, int q, int dir) {
    int best = -1;
    for (int r = 0; r < s.n; ++r) {
        if ((s.flags[r] & kGfDup) || r == p || r == q) continue;
        const long long o = gf_orient(s, p, q, r);
        if (dir > 0 ? o <= 0 : o >= 0) continue;
        if (best < 0) { best = r; continue; }
        const int ic = dir > 0 ? gf_incircle(s, p, q, best, r) : gf_incircle(s, p, best, q, r);
        if (ic > 0) best = r;
        else if (ic == 0) {
            const long long o2 = gf_orient(s, p, best, r);
            if (dir > 0 ? o2 > 0 : o2 < 0) best = r;
        }
    }
    return best;
}

// The executors' decline: the lowest status of a phase wins, on both sides
template <class X>
MRG_GF_HD void gf_settle(X& x, GfNear& s, int status) { x.lower(&s.status, status); }

// The status as every lane sees it between two phases: the barrier in front of the read ends the phase that may have
// lowered it, the one behind it keeps the next phase from lowering it under a lane that has not read it yet (lanes that
// disagreed would part ways at the next barrier)
template <class X>
MRG_GF_HD int gf_status(X& x, const GfNear& s) {
    x.barrier();
    const int status = s.status;
    x.barrier();
    return status;
}

// PHASE 2, one site: its ring.  From the nearest site -- always a neighbour -- counter-clockwise until the ring closes;
// at a gap (a hull site) the ring is walked again, clockwise from the neighbour in front of the gap to the one behind
// it, and turned round: it then begins behind the gap, and its last step is the one across it.
template <class X>
MRG_GF_HD void gf_ring_of_site(X& x, GfNear& s, GfFar& g, int p) {
    s.deg[p] = 0;
    s.hull[p] = 0;
    if (s.flags[p] & kGfDup) return;
    int q0 = -1;
    long long best = 0;
    for (int r = 0; r < s.n; ++r) {
        if ((s.flags[r] & kGfDup) || r == p) continue;
        const long long dx = (long long)s.sx[r] - s.sx[p], dy = (long long)s.sy[r] - s.sy[p];
        const long long d2 = dx * dx + dy * dy;
        if (q0 < 0 || d2 < best) { q0 = r; best = d2; }
    }
    if (q0 < 0) return;
    uint16_t* ring = g.ring + (size_t)p * kGfRingCap;
    int deg = 0, q = q0;
    bool gap = false;
    for (;;) {  // (at most kGfRingCap rounds)
        if (deg == kGfRingCap) { gf_settle(x, s, kGfDeclineTable); return; }
        ring[deg++] = (uint16_t)q;
        const int nx = gf_next_neighbour(s, p, q, +1);
        if (nx == q0) break;
        if (nx < 0) { gap = true; break; }
        q = nx;
    }
    if (gap) {
        deg = 0;
        for (;;) {
            if (deg == kGfRingCap) { gf_settle(x, s, kGfDeclineTable); return; }
            ring[deg++] = (uint16_t)q;
            const int nx = gf_next_neighbour(s, p, q, -1);
            if (nx < 0) break;
            q = nx;
        }
        for (int i = 0, j = deg - 1; i < j; ++i, --j) {
            const uint16_t t = ring[i];
            ring[i] = ring[j];
            ring[j] = t;
        }
        s.hull[p] = 1;
    }
    s.deg[p] = (uint16_t)deg;
}

// PHASES 3 and 4, one site: its adjacency entries in the visiting order of for_each_adjacent (grid.cpp:392-431) under
// canonical_start, `tri` and `far` read off the neighbour's ring by the generic rule (grid.cpp:373-383; a hull site's step
// across its gap closes no triangle, grid.cpp:360-362).  Returns their number; writes them from entry `at` on if asked.
template <class X>
MRG_GF_HD int gf_adjacency_of_site(X& x, GfNear& s, GfFar& g, int c, bool write, int at) {
    const int deg = s.deg[c];
    if (deg == 0) return 0;
    const uint16_t* ring = g.ring + (size_t)c * kGfRingCap;
    const long long px = s.sx[c], py = s.sy[c];
    int start = 0;
    for (int k = 1; k < deg; ++k) {  // the neighbour with the smallest direction angle in [0, 2 pi) from +x
        const long long ax = s.sx[ring[k]] - px, ay = s.sy[ring[k]] - py;
        const long long bx = s.sx[ring[start]] - px, by = s.sy[ring[start]] - py;
        const bool ha = !(ay > 0 || (ay == 0 && ax > 0)), hb = !(by > 0 || (by == 0 && bx > 0));
        if (ha != hb ? hb : ax * by - ay * bx > 0) start = k;
    }
    int count = 0;
    auto emit = [&](int site, long long dx, long long dy) {
        if (write && at + count < kGfMaxAdj) {
            const int e = at + count;
            g.a_site[e] = (uint16_t)site;
            g.a_src[e] = (uint16_t)c;
            g.a_dx[e] = (int32_t)dx;
            g.a_dy[e] = (int32_t)dy;
            g.a_len[e] = sqrt((double)(dx * dx + dy * dy));  // exact sum, correctly rounded root
        }
        ++count;
    };
    for (int kk = 0; kk < deg; ++kk) {
        const int k = (kk + start) % deg;
        const int b = ring[k];
        const long long v0x = s.sx[b] - px, v0y = s.sy[b] - py;
        emit(b, v0x, v0y);
        if (deg < 2) continue;
        const int cn = ring[(k + 1) % deg];
        const long long v1x = s.sx[cn] - px, v1y = s.sy[cn] - py;
        if (v1x * v0y > v0x * v1y) continue;  // not an acute turn: graph boundary (:116-117)
        if (s.hull[c] && k == deg - 1) continue;
        // what precedes c in the ring of b is cn (:123); what precedes cn there is the in-between site (:127)
        const uint16_t* rb = g.ring + (size_t)b * kGfRingCap;
        const int degb = s.deg[b];
        int p = 0;
        while (p < degb && rb[p] != c) ++p;
        if (p == degb) { gf_settle(x, s, kGfDeclineRing); continue; }
        if (rb[(p + degb - 1) % degb] != cn) continue;
        const int d = rb[(p + 2 * degb - 2) % degb];
        const long long vmx = s.sx[d] - px, vmy = s.sy[d] - py;
        if (v1x * vmy > vmx * v1y) continue;  // must lie angularly between its neighbours (:128-131)
        if (vmx * v0y > v0x * vmy) continue;
        emit(d, vmx, vmy);
    }
    return count;
}

// PHASE 5: the walk of walk_sequence / next_along_sequence (grid.cpp:482-560): n_remaining steps, each to the FIRST
// adjacency entry of the site that continues the sequence.  Every comparison it evaluates against a threshold is made
// with the guard band; one inside the band declines the list.  `path`: the sites visited, if given.  Returns the last
// site, or -1.
template <class X>
MRG_GF_HD int gf_walk(X& x, GfNear& s, const GfFar& g, int e0, int n_remaining, double band, int32_t* path) {
    double lx = (double)g.a_dx[e0], ly = (double)g.a_dy[e0], last_len = g.a_len[e0], ratio_sum = 0.0;
    int ratio_n = 0, c = g.a_site[e0], last = -1;
    auto near_to = [&](double v, double threshold) { return v > threshold - band && v < threshold + band; };
    for (int i = 0; i < n_remaining; ++i) {
        int chosen = -1;
        double chosen_ratio = 0.0;
        const int e1 = s.adj_off[c + 1];
        for (int e = s.adj_off[c]; e < e1; ++e) {
            const double dx = (double)g.a_dx[e], dy = (double)g.a_dy[e], len = g.a_len[e];
            const double dot = lx * dx + ly * dy;  // (exact: two products below 2^50)
            const double den = last_len * len;
            // most neighbours point somewhere else entirely: decided without the division wherever the quotient is
            // further below the threshold than the band and any rounding
            if (dot < (kGfSpacingCos - 2.0 * band - 1e-6) * den) continue;
            const double cos_err = dot / den;
            if (near_to(cos_err, kGfSpacingCos)) gf_settle(x, s, kGfDeclineGuard);
            if (cos_err < kGfSpacingCos) continue;
            const double ratio = len / last_len;
            if (near_to(ratio, kGfRatioMin) || near_to(ratio, kGfRatioMax)) gf_settle(x, s, kGfDeclineGuard);
            if (ratio < kGfRatioMin || ratio > kGfRatioMax) continue;
            if (ratio_n > 2) {
                const double dev = ratio - ratio_sum / (double)ratio_n;
                if (near_to(dev, -kGfRatioDev) || near_to(dev, kGfRatioDev)) gf_settle(x, s, kGfDeclineGuard);
                if (dev < -kGfRatioDev || dev > kGfRatioDev) continue;
            }
            chosen = e;
            chosen_ratio = ratio;
            break;  // the first match (:216-222)
        }
        if (chosen < 0) return -1;
        ratio_sum += chosen_ratio;
        ratio_n++;
        lx = (double)g.a_dx[chosen];
        ly = (double)g.a_dy[chosen];
        last_len = g.a_len[chosen];
        last = c = g.a_site[chosen];
        if (path) path[i] = c;
    }
    return last;
}

// is_crossing, find_grid.cc:780-823 (single precision, like the reference; grid.cpp: segments_cross)
MRG_GF_HD bool gf_segments_cross(const GfNear& s, int a0, int a1, int b0, int b1) {
    const float l0[2] = {(float)(s.sx[a1] - s.sx[a0]), (float)(s.sy[a1] - s.sy[a0])};
    const float q0[2] = {(float)(s.sx[b0] - s.sx[a0]), (float)(s.sy[b0] - s.sy[a0])};
    const float q1[2] = {(float)(s.sx[b1] - s.sx[a0]), (float)(s.sy[b1] - s.sy[a0])};
    const float d2 = l0[0] * l0[0] + l0[1] * l0[1];
    const float r0[2] = {q0[0] * l0[0] + q0[1] * l0[1], -q0[0] * l0[1] + q0[1] * l0[0]};
    const float r1[2] = {q1[0] * l0[0] + q1[1] * l0[1], -q1[0] * l0[1] + q1[1] * l0[0]};
    if (r0[1] * r1[1] > 0) return false;
    if ((r0[0] < 0 && r1[0] < 0) || (r0[0] > d2 && r1[0] > d2)) return false;
    const float k = r0[1] / (r0[1] - r1[1]);
    const float xx = r0[0] + k * (r1[0] - r0[0]);
    return xx >= 0.0f && xx <= d2;
}

// next_outer_edge, find_grid.cc:825-951 (grid.cpp: CycleSearch::extend), one function per depth instead of a recursion.
// An outer edge is a position in s.outer; its sequence's ends:
MRG_GF_HD int gf_oc0(const GfNear& s, int pos) { return s.seq_c0[s.outer[pos]]; }
MRG_GF_HD int gf_ocl(const GfNear& s, int pos) { return s.seq_cl[s.outer[pos]]; }
MRG_GF_HD bool gf_extend3(const GfNear& s, int e[4], int start_site) {
    const int cur = e[2];
    const int q1 = s.out_off[gf_ocl(s, cur) + 1];
    for (int pos = s.out_off[gf_ocl(s, cur)]; pos < q1; ++pos) {
        if (gf_ocl(s, pos) == gf_oc0(s, cur)) continue;  // straight back
        if (gf_ocl(s, pos) != start_site) continue;
        if (gf_segments_cross(s, gf_oc0(s, e[1]), gf_ocl(s, e[1]), gf_oc0(s, pos), gf_ocl(s, pos))) return false;
        e[3] = pos;
        return true;
    }
    return false;
}
MRG_GF_HD bool gf_extend2(const GfNear& s, int e[4], int start_site) {
    const int cur = e[1];
    bool found = false;
    int best[4] = {0, 0, 0, 0};
    const int q1 = s.out_off[gf_ocl(s, cur) + 1];
    for (int pos = s.out_off[gf_ocl(s, cur)]; pos < q1; ++pos) {
        if (gf_ocl(s, pos) == gf_oc0(s, cur)) continue;
        if (gf_ocl(s, pos) == start_site) continue;
        if (gf_segments_cross(s, gf_oc0(s, e[0]), gf_ocl(s, e[0]), gf_oc0(s, pos), gf_ocl(s, pos))) continue;
        e[2] = pos;
        if (!gf_extend3(s, e, start_site)) continue;
        if (found) return false;  // must be unique
        found = true;
        for (int k = 0; k < 4; ++k) best[k] = e[k];
    }
    if (!found) return false;
    for (int k = 0; k < 4; ++k) e[k] = best[k];
    return true;
}
MRG_GF_HD bool gf_extend1(const GfNear& s, int e[4], int start_site) {
    const int cur = e[0];
    bool found = false;
    int best[4] = {0, 0, 0, 0};
    const int q1 = s.out_off[gf_ocl(s, cur) + 1];
    for (int pos = s.out_off[gf_ocl(s, cur)]; pos < q1; ++pos) {
        if (gf_ocl(s, pos) == gf_oc0(s, cur)) continue;
        if (gf_ocl(s, pos) == start_site) continue;
        e[1] = pos;
        if (!gf_extend2(s, e, start_site)) continue;
        if (found) return false;
        found = true;
        for (int k = 0; k < 4; ++k) best[k] = e[k];
    }
    if (!found) return false;
    for (int k = 0; k < 4; ++k) e[k] = best[k];
    return true;
}

// the first sequence from `from` to `to`, or -1 (grid.cpp: seq_from_to)
MRG_GF_HD int gf_seq_from_to(const GfNear& s, int from, int to) {
    for (int q = s.seq_off[from]; q < s.seq_off[from + 1]; ++q)
        if (s.seq_cl[q] == to) return q;
    return -1;
}

// the gridn sites of a sequence into `out` (grid.cpp: sequence_points): its walk again, the same decisions
template <class X>
MRG_GF_HD bool gf_sequence_points(X& x, GfNear& s, const GfFar& g, int q, double band, int32_t* out) {
    const int e = g.seq_e[q];
    out[0] = s.seq_c0[q];
    out[1] = g.a_site[e];
    return s.gridn == 2 || gf_walk(x, s, g, e, s.gridn - 2, band, out + 2) >= 0;
}

// PHASE 6, one lane: grid.cpp:851-1022 -- outer edges, unique 4-cycles, the one equal-and-opposite pair, the clockwise
// cycle and its top edge, the rows.  Writes the board's candidate indices and settles the status.
template <class X>
MRG_GF_HD void gf_tail(X& x, GfNear& s, const GfFar& g, double band, int32_t* index) {
    const int gridn = s.gridn, n = s.n;
    // outer-edge candidates: sequences whose start site starts at least two (:1246-1262); they stay in site order
    int nouter = 0;
    for (int c = 0; c < n; ++c) {
        s.out_off[c] = (uint16_t)nouter;
        if (s.seq_off[c + 1] - s.seq_off[c] < 2) continue;
        for (int q = s.seq_off[c]; q < s.seq_off[c + 1]; ++q) {
            if (nouter == kGfMaxOuter) { gf_settle(x, s, kGfDeclineTable); return; }
            s.used[nouter] = 0;
            s.outer[nouter++] = (uint16_t)q;
        }
    }
    s.out_off[n] = (uint16_t)nouter;
    s.nouter = nouter;
    if (nouter < 8) { gf_settle(x, s, kGfNone); return; }
    // 4-cycles of outer edges (:1287-1322)
    int ncyc = 0;
    for (int i = 0; i < nouter; ++i) {
        if (s.used[i]) continue;
        int e[4] = {i, 0, 0, 0};
        if (!gf_extend1(s, e, gf_oc0(s, i))) continue;
        if (ncyc == kGfMaxCycles) { gf_settle(x, s, kGfDeclineTable); return; }
        for (int k = 0; k < 4; ++k) {
            s.cyc[ncyc][k] = (uint16_t)e[k];
            s.used[e[k]] = 1;
        }
        ++ncyc;
    }
    if (ncyc < 2) { gf_settle(x, s, kGfNone); return; }
    // exactly one equal-and-opposite pair (:953-1003, :1324-1352)
    int pair[2] = {-1, -1};
    for (int i0 = 0; i0 < ncyc; ++i0)
        for (int i1 = i0 + 1; i1 < ncyc; ++i1) {
            const uint16_t* a = s.cyc[i0];
            const uint16_t* b = s.cyc[i1];
            int ia = 0, ib = -1;
            const int p0 = gf_oc0(s, a[0]);
            for (int k = 0; k < 4; ++k)
                if (gf_ocl(s, b[k]) == p0) { ib = k; break; }
            if (ib < 0) continue;
            bool opposite = true;
            for (int i = 0; i < 4 && opposite; ++i) {
                if (gf_oc0(s, a[ia]) != gf_ocl(s, b[ib]) || gf_ocl(s, a[ia]) != gf_oc0(s, b[ib])) opposite = false;
                ia = (ia + 1) % 4;
                ib = (ib + 3) % 4;
            }
            if (!opposite) continue;
            if (pair[0] >= 0) { gf_settle(x, s, kGfNone); return; }
            pair[0] = i0;
            pair[1] = i1;
        }
    if (pair[0] < 0) { gf_settle(x, s, kGfNone); return; }
    // clockwise cycle and its top edge (:1025-1190)
    const uint16_t* cyc2[2] = {s.cyc[pair[0]], s.cyc[pair[1]]};
    int sign = 0;
    for (int i0 = 0; i0 < 4; ++i0) {
        const int i1 = (i0 + 1) % 4;
        const int a = cyc2[0][i0], b = cyc2[0][i1];
        const int v0x = (s.sx[gf_ocl(s, a)] - s.sx[gf_oc0(s, a)]) / 1024, v0y = (s.sy[gf_ocl(s, a)] - s.sy[gf_oc0(s, a)]) / 1024;  // FIND_GRID_SCALE_APPROX_POWER2
        const int v1x = (s.sx[gf_ocl(s, b)] - s.sx[gf_oc0(s, b)]) / 1024, v1y = (s.sy[gf_ocl(s, b)] - s.sy[gf_oc0(s, b)]) / 1024;
        sign |= (int)((long long)v1x * v0y < (long long)v0x * v1y) << i0;
    }
    int iclockwise;
    if (sign == 15) iclockwise = 0;
    else if (sign == 0) iclockwise = 1;
    else { gf_settle(x, s, kGfNone); return; }  // not convex
    int itop[2];
    for (int ic = 0; ic < 2; ++ic) {
        int ymin[2] = {INT32_MAX, INT32_MAX}, emin[2] = {-1, -1}, plo[2] = {0, 0}, phi[2] = {0, 0};
        for (int i = 0; i < 4; ++i) {
            const int c0 = gf_oc0(s, cyc2[ic][i]), cl = gf_ocl(s, cyc2[ic][i]);
            int y_here, lo, hi;
            if (s.sy[c0] < s.sy[cl]) { y_here = s.sy[c0]; lo = c0; hi = cl; }
            else { y_here = s.sy[cl]; lo = cl; hi = c0; }
            if (y_here < ymin[0]) {
                ymin[1] = ymin[0]; emin[1] = emin[0]; plo[1] = plo[0]; phi[1] = phi[0];
                ymin[0] = y_here; emin[0] = i; plo[0] = lo; phi[0] = hi;
            } else if (y_here < ymin[1]) {
                ymin[1] = y_here; emin[1] = i; plo[1] = lo; phi[1] = hi;
            }
        }
        long long v0y = (s.sy[phi[0]] - s.sy[plo[0]]) / 1024, v0x = (s.sx[phi[0]] - s.sx[plo[0]]) / 1024;
        long long v1y = (s.sy[phi[1]] - s.sy[plo[1]]) / 1024, v1x = (s.sx[phi[1]] - s.sx[plo[1]]) / 1024;
        v0x = v0x > 0 ? v0x : -v0x;
        v1x = v1x > 0 ? v1x : -v1x;
        const long long cr = (v0x * v1y - v0y * v1x) * (v0x * v1y - v0y * v1x);
        const long long den = (v0x * v0x + v0y * v0y) * (v1x * v1x + v1y * v1y);
        if ((cr > 0 ? cr : -cr) * 8 < den * 1) { gf_settle(x, s, kGfNone); return; }  // the two highest edges are too parallel (:1153-1156)
        const long long l = v0y * v1x, rr = v1y * v0x;
        itop[ic] = ((l > 0 ? l : -l) < (rr > 0 ? rr : -rr)) ? emin[0] : emin[1];
    }
    // rows between the two vertical outer edges (:1378-1440)
    int32_t* lp = s.tmp;
    int32_t* rp = s.tmp + kGfMaxGridn;
    int32_t* rows = s.tmp + 2 * kGfMaxGridn;
    int32_t* row = s.tmp + 3 * kGfMaxGridn;
    rows[0] = s.outer[cyc2[iclockwise][itop[iclockwise]]];
    const int vleft = s.outer[cyc2[1 - iclockwise][(itop[1 - iclockwise] + 1) % 4]];
    const int vright = s.outer[cyc2[iclockwise][(itop[iclockwise] + 1) % 4]];
    if (!gf_sequence_points(x, s, g, vleft, band, lp) || !gf_sequence_points(x, s, g, vright, band, rp)) { gf_settle(x, s, kGfNone); return; }
    for (int i = 1; i < gridn; ++i) {
        rows[i] = gf_seq_from_to(s, lp[i], rp[i]);
        if (rows[i] < 0 || gf_seq_from_to(s, rp[i], lp[i]) < 0) { gf_settle(x, s, kGfNone); return; }
    }
    // (every row is looked at before the first index is written: a list without a board leaves none)
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < gridn; ++i) {
            if (!gf_sequence_points(x, s, g, rows[i], band, row)) { gf_settle(x, s, kGfNone); return; }
            if (pass)
                for (int j = 0; j < gridn; ++j) index[i * gridn + j] = s.orig[row[j]];
        }
    if (s.status == kGfRunning) s.status = kGfFound;
}

// One list, all phases.  xy: the list's candidates (count of them read), index: its gridn^2 outputs (-1 where there is
// no board).  Returns the status on every lane.
template <class X>
MRG_GF_HD int gf_find_grid(X& x, GfNear& s, GfFar& g, const int32_t* xy, int count, int capacity, int gridn, int guard_bits,
                           int32_t* index) {
    const int lane = x.lane(), lanes = x.lanes();
    int st;
    const double band = ldexp(1.0, -guard_bits);
    int32_t* const rx = s.rx;
    int32_t* const ry = s.ry;
    // PHASE 1: load, order, duplicates
    for (int i = lane; i < gridn * gridn; i += lanes) index[i] = -1;
    if (lane == 0) {
        s.status = kGfRunning;
        s.gridn = gridn;
        s.n = 0;
        if (count < 0 || count > capacity || count > kGfMaxSites) s.status = kGfDeclineCount;
        else if (count < gridn * gridn) s.status = kGfNone;
        else s.n = count;
    }
    if ((st = gf_status(x, s)) != kGfRunning) return st;
    const int n = s.n;
    for (int i = lane; i < n; i += lanes) {
        const int vx = xy[2 * i], vy = xy[2 * i + 1];
        rx[i] = vx;
        ry[i] = vy;
        if (vx <= -kGfCoordLimit || vx >= kGfCoordLimit || vy <= -kGfCoordLimit || vy >= kGfCoordLimit) gf_settle(x, s, kGfDeclineCoord);
    }
    if ((st = gf_status(x, s)) != kGfRunning) return st;
    for (int i = lane; i < n; i += lanes) {  // the site's place in boost's cell order: (x, y), then the candidate index
        const int vx = rx[i], vy = ry[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const int ux = rx[j], uy = ry[j];
            rank += ux != vx ? ux < vx : (uy != vy ? uy < vy : j < i);
        }
        s.sx[rank] = vx;
        s.sy[rank] = vy;
        s.orig[rank] = (uint16_t)i;
    }
    x.barrier();
    for (int i = lane; i < n; i += lanes) s.flags[i] = i > 0 && s.sx[i] == s.sx[i - 1] && s.sy[i] == s.sy[i - 1] ? kGfDup : 0;
    x.barrier();
    if (lane == 0) {  // fewer than three distinct sites, or all of them on one line: no triangle, no board (grid.cpp:121-125)
        int s1 = -1;
        bool plane = false;
        for (int k = 1; k < n && !plane; ++k) {
            if (s.flags[k] & kGfDup) continue;
            if (s1 < 0) s1 = k;
            else plane = gf_orient(s, 0, s1, k) != 0;
        }
        if (!plane) s.status = kGfNone;
    }
    if ((st = gf_status(x, s)) != kGfRunning) return st;
    // PHASE 2: Voronoi neighbour rings
    for (int p = lane; p < n; p += lanes) gf_ring_of_site(x, s, g, p);
    if ((st = gf_status(x, s)) != kGfRunning) return st;
    // PHASES 3 and 4: tri / far, adjacency lists -- counted, placed, written
    for (int c = lane; c < n; c += lanes) s.seq_off[c] = (uint16_t)gf_adjacency_of_site(x, s, g, c, false, 0);
    x.barrier();
    if (lane == 0) {
        int at = 0;
        for (int c = 0; c < n; ++c) {
            s.adj_off[c] = (uint16_t)(at < kGfMaxAdj ? at : kGfMaxAdj);
            at += s.seq_off[c];
        }
        s.adj_off[n] = (uint16_t)(at < kGfMaxAdj ? at : kGfMaxAdj);
        s.nadj = at;
        if (at > kGfMaxAdj) gf_settle(x, s, kGfDeclineTable);
    }
    if ((st = gf_status(x, s)) != kGfRunning) return st;
    for (int c = lane; c < n; c += lanes) gf_adjacency_of_site(x, s, g, c, true, s.adj_off[c]);
    x.barrier();
    // PHASE 5: one walk per adjacency entry, then the sequences in (site order, entry order)
    const int nadj = s.nadj;
    for (int e = lane; e < nadj; e += lanes) {
        const int clast = gf_walk(x, s, g, e, gridn - 2, band, nullptr);
        g.a_clast[e] = clast < 0 ? kGfNoSite : (uint16_t)clast;
    }
    if ((st = gf_status(x, s)) != kGfRunning) return st;
    const int chunk = (nadj + lanes - 1) / lanes;
    for (int l = lane; l < lanes; l += lanes) {
        int found = 0;
        for (int e = l * chunk; e < (l + 1) * chunk && e < nadj; ++e) found += g.a_clast[e] != kGfNoSite;
        s.tmp[l] = found;
    }
    x.barrier();
    if (lane == 0) {
        int at = 0;
        for (int l = 0; l < lanes; ++l) {
            const int found = s.tmp[l];
            s.tmp[l] = at;
            at += found;
        }
        s.nseq = at;
        if (at > kGfMaxSeq) gf_settle(x, s, kGfDeclineTable);
    }
    if ((st = gf_status(x, s)) != kGfRunning) return st;
    for (int l = lane; l < lanes; l += lanes) {
        int at = s.tmp[l];
        for (int e = l * chunk; e < (l + 1) * chunk && e < nadj; ++e) {
            if (g.a_clast[e] == kGfNoSite) continue;
            s.seq_c0[at] = g.a_src[e];
            s.seq_cl[at] = g.a_clast[e];
            g.seq_e[at] = (uint16_t)e;
            ++at;
        }
    }
    x.barrier();
    if (lane == 0) {  // the sequences of a site are one run
        const int nseq = s.nseq;
        int q = 0;
        for (int c = 0; c < n; ++c) {
            s.seq_off[c] = (uint16_t)q;
            while (q < nseq && s.seq_c0[q] == c) ++q;
        }
        s.seq_off[n] = (uint16_t)q;
        // PHASE 6
        gf_tail(x, s, g, band, index);
    }
    return gf_status(x, s);
}

}  // namespace mrg
