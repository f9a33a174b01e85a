// Blob path, rows a-19 / (f)-4: mrgingham's find_blobs_from_image_array (find_blobs.cc:14-46) = a
// cv::SimpleBlobDetector (minArea 20, maxArea 80000, minDistBetweenBlobs 5, dark blobs, everything else at
// its default) whose keypoints become (int)(x * 1000 + 0.5) candidates for the grid finder.
//
// OpenCV arithmetic throughout (parity unpinned, like the other OpenCV steps): restated from its published
// algorithm -- threshold sweep 50..210 step 10, cv::findContours(RETR_LIST, CHAIN_APPROX_NONE) per
// threshold (Suzuki-Abe border following), per contour the moment / inertia / convexity / colour filters,
// median radius, grouping of the centres across thresholds (blobdetector.cpp, contours.cpp, moments.cpp).
//
// Split: the device does what touches every pixel -- the 17 binarised bit planes in one pass over the frame, the
// border start candidates of every plane and the border following itself (in parallel: arcs between candidates,
// then pointer jumping over the cycles of arcs, see below), with the contour-area sum of contourMoments (Green's
// theorem: exact in integers, order-independent) for the area filter.  Borders that pass it get their points
// written, every arc its own stretch, with the other five moment sums (integers too) and the pixel at the rounded
// centre that the colour filter asks for.  The host finishes the few survivors in double precision (inertia, convex
// hull, colour, median radius, grouping) and needs no copy of the pixels: microseconds, like the grid finder that
// consumes the result.
//
// ONE pipeline for one frame and for a batch: a chunk of frames is `frames x 17` bit planes in one node space (plane =
// frame * 17 + threshold), every kernel is launched once per chunk, and the one-frame entry (blob_detect) is the chunk
// of one frame.  See blob_detect_batch.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "ctx.h"

namespace mrg {

namespace {

constexpr int kNumThresh = 17;            // 50, 60, .. 210 (minThreshold 50, maxThreshold 220, step 10)
constexpr int kThresh0 = 50, kThreshStep = 10;

struct BitPlanes {
    const uint32_t* bits;  // [planes][h][wpr], plane = frame * kNumThresh + threshold
    int w, h, wpr;
};

// The device words of one chunk of `nf` frames (P = nf * kNumThresh planes); the host reads all of them in one copy.
struct BlobCounters {
    int* err;         // [nf]  != 0: the frame has a border arc longer than kMaxArc
    int* plane_cnt;   // [P]   nodes of the plane
    int* plane_base;  // [P]   first node of the plane
    int* rec_cnt;     // [nf]  contours of the frame that pass the area filter ...
    int* pts_cnt;     // [nf]  ... and their points
    int* rec_base;    // [nf]  first record / first point of the frame in the chunk's arrays
    int* pts_base;    // [nf]
    int* rec_cur;     // [nf]  write cursors within the frame's stretch
    int* pts_cur;     // [nf]
};
constexpr int blob_counter_words(int nf) { return nf * (7 + 2 * kNumThresh); }

// direction codes of the border follower: 0 = +x, then counter-clockwise on the screen (y down)
__device__ __constant__ int kDX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
__device__ __constant__ int kDY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

// first set direction going clockwise (decreasing code) from `from` (exclusive, wrapping back to it); -1 if none
__device__ __forceinline__ int first_cw(uint32_t m, int from) {
    if (!m) return -1;
    // rotate so that direction from-1 becomes bit 7, from-2 bit 6, ...: bit (7 - k) <-> direction from-1-k
    const uint32_t r = ((m | (m << 8)) >> (from & 7)) & 0xffu;  // bit j = direction from + j; from-1-k = from + (7-k)
    return (from + (31 - __clz((int)r))) & 7;
}
// first set direction going counter-clockwise (increasing code) from s + 1
__device__ __forceinline__ int first_ccw(uint32_t m, int s) {
    const uint32_t r = ((m | (m << 8)) >> ((s + 1) & 7)) & 0xffu;  // bit j = direction s + 1 + j
    return (s + 1 + (__ffs((int)r) - 1)) & 7;
}

// one thread = 32 pixels of a row of frame blockIdx.z -> one word of each of the frame's 17 planes
__global__ __launch_bounds__(256) void blob_bitplanes_kernel(const uint8_t* img, long long frame_pitch, int stride, int w, int h,
                                                             int wpr, uint32_t* bits) {
    const int wx = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (wx >= wpr) return;
    img += f * frame_pitch;
    bits += (long long)f * kNumThresh * h * wpr;
    uint32_t word[kNumThresh];
#pragma unroll
    for (int t = 0; t < kNumThresh; ++t) word[t] = 0;
    const uint8_t* row = img + (long long)y * stride;
    for (int i = 0; i < 32; ++i) {
        const int x = wx * 32 + i;
        if (x >= w) break;
        const int v = row[x];
#pragma unroll
        for (int t = 0; t < kNumThresh; ++t) word[t] |= (uint32_t)(v > kThresh0 + kThreshStep * t) << i;  // THRESH_BINARY
    }
#pragma unroll
    for (int t = 0; t < kNumThresh; ++t) bits[((long long)t * h + y) * wpr + wx] = word[t];
}

// ---------------------------------------------------------------------------------------------
// Border following, in parallel.  The sequential algorithm (icvFetchContour, CHAIN_APPROX_NONE) walks a border
// pixel by pixel; the state of the walk is (pixel, direction of the pixel it came from) and the next state is a
// function of the state and the pixel's 8 neighbours.  The raster scan starts a walk at a white pixel whose left
// neighbour is 0 (outer-type start) or whose right neighbour is 0 (hole-type start), in the state the start rule
// gives it -- and EVERY left-edge / right-edge pixel of a border is such a start candidate whose start state lies
// on that border's cycle of states.  So the candidates cut every border into ARCS: a lane walks from its
// candidate only to the next candidate state it meets (whatever its key), a handful of steps except along
// horizontal runs, and leaves (next candidate, steps, the arc's share of the contour area sum).  Then the cycles
// of `next` are reduced with pointer jumping: the smallest candidate of a cycle is the start the raster scan
// would have used (the owner; its key orders the contours), a list ranking from it gives every arc its offset in
// the contour's point list and the owner the totals.  Round 2 walked every border end to end in one lane from
// every candidate (20-65 ms per 12 MP frame, a launch lasting as long as its longest border, and give-up rules
// for borders of more than 65 536 steps); this is O(log) rounds over short arcs and needs no give-up rule.
//
// Candidates are numbered in raster order per plane (row offsets + per-word prefix counts + popcounts, no atomics,
// no sort), planes one after the other: node = candidate = arc.  Two candidates at one pixel with the same start
// state (a one-pixel-wide stroke: left AND right neighbour 0) are the same state; the outer-type one is the node,
// the hole-type one is dead (contours.cpp: the outer check comes first and marks the pixel).
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kNoNode = 0xffffffffu;
constexpr int kMaxArc = 1 << 20;  // steps; an arc is bounded by the longest horizontal run of a border (the frame's width)

// candidate masks of one word of a row: bit i = pixel 32 * wx + i starts an outer-type / a hole-type border walk
__device__ __forceinline__ void word_candidates(uint32_t cur, uint32_t left_in, uint32_t right_in, int wx, int w,
                                                uint32_t& outer, uint32_t& hole) {
    outer = cur & ~((cur << 1) | left_in);
    hole = cur & ~((cur >> 1) | (right_in << 31));
    (void)wx;
    (void)w;
}
// The raster scan never looks at the zero pad, so a white pixel of the LAST COLUMN is no hole-type start.  It is kept
// as a node all the same -- it cuts the walk down the frame's right edge into arcs like every other candidate (without
// it that is one arc of `height` vertical steps, a row load each: 2.5 ms at 3072 rows, the whole launch) -- but it can
// never own a border: it does not take part in the election of the smallest node.
__device__ __forceinline__ bool pseudo_node(uint32_t key, int w) { return (key & 1u) && (int)((key >> 1) & 0x7fffu) == w - 1; }

// rows y-1, y, y+1 around word wx of plane t, each as 34 bits: bit 0 = the previous word's bit 31, bits 1..32 = the
// word, bit 33 = the next word's bit 0.  A walk reloads a row only when it leaves the word or changes row.
struct BlobWin {
    int wx, y;
    unsigned long long r[3];
};
__device__ __forceinline__ unsigned long long row34(const BitPlanes& bp, int t, int wx, int y) {
    if ((unsigned)y >= (unsigned)bp.h) return 0ull;
    const uint32_t* row = bp.bits + ((long long)t * bp.h + y) * bp.wpr;
    const uint32_t cur = row[wx];
    const uint32_t prev = wx > 0 ? row[wx - 1] : 0u, next = wx + 1 < bp.wpr ? row[wx + 1] : 0u;
    return (unsigned long long)(prev >> 31) | ((unsigned long long)cur << 1) | ((unsigned long long)(next & 1u) << 33);
}
__device__ __forceinline__ void win_goto(BlobWin& wn, const BitPlanes& bp, int t, int x, int y) {
    const int wx = x >> 5;
    if (wx == wn.wx && y == wn.y) return;
    if (wx == wn.wx && y == wn.y + 1) {
        wn.r[0] = wn.r[1]; wn.r[1] = wn.r[2]; wn.r[2] = row34(bp, t, wx, y + 1);
    } else if (wx == wn.wx && y == wn.y - 1) {
        wn.r[2] = wn.r[1]; wn.r[1] = wn.r[0]; wn.r[0] = row34(bp, t, wx, y - 1);
    } else {
        wn.r[0] = row34(bp, t, wx, y - 1); wn.r[1] = row34(bp, t, wx, y); wn.r[2] = row34(bp, t, wx, y + 1);
    }
    wn.wx = wx;
    wn.y = y;
}
// the 8 neighbours of pixel x of the window's centre row as a mask, bit s = the pixel in direction s
__device__ __forceinline__ uint32_t win_neighbours(const BlobWin& wn, int x) {
    const int b = x & 31;
    const uint32_t up = (uint32_t)(wn.r[0] >> b) & 7u, mid = (uint32_t)(wn.r[1] >> b) & 7u, dn = (uint32_t)(wn.r[2] >> b) & 7u;
    return ((mid >> 2) & 1u) | (((up >> 2) & 1u) << 1) | (((up >> 1) & 1u) << 2) | ((up & 1u) << 3) |
           ((mid & 1u) << 4) | ((dn & 1u) << 5) | (((dn >> 1) & 1u) << 6) | (((dn >> 2) & 1u) << 7);
}

struct BlobNodes {         // per node (= candidate = arc), N of them; planes one after the other, raster order within a plane
    uint32_t* key;         // (y << 16) | (x << 1) | type
    uint32_t* next;        // the node whose start state the arc ends in (itself: a border of one arc; a dead node: itself)
    unsigned long long* a00;  // the arc's share of the contourMoments sum a00 (wrap-around)
    uint32_t* n;           // steps = points of the arc; 0 = dead node
    uint32_t* jmp;         // pointer jumping (leader rounds); afterwards, at the owner: the contour's record
    uint32_t* leader;      // the smallest node of the cycle
    uint32_t* ptr[2];      // list ranking (double-buffered): successor 2^r arcs on, kNoNode at the end of the list
    unsigned long long* sa[2];  // ... a00 summed from this arc to the end of the list
    uint32_t* sn[2];       // ... points from this arc to the end of the list
    int32_t* off;          // per node: first point of its contour in the point arena (at the owner; -1: contour rejected)
    uint16_t* plane;       // the node's plane within the chunk
};
constexpr size_t kBlobNodeBytes = 4 + 4 + 8 + 4 + 4 + 4 + 8 + 16 + 8 + 4 + 2;  // 66
constexpr int kMaxChunkFrames = 65535 / kNumThresh;  // (plane ids are 16 bits, and a grid dimension)

// pass 1: candidates per word (exclusive prefix within the row) and per row.  One workgroup per (row, plane of the chunk).
__global__ __launch_bounds__(256) void blob_count_kernel(BitPlanes bp, uint32_t* wordpre, uint32_t* rowcnt) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t carry;
    const int y = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const uint32_t* row = bp.bits + ((long long)t * bp.h + y) * bp.wpr;
    uint32_t* pre = wordpre + ((long long)t * bp.h + y) * bp.wpr;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int w0 = 0; w0 < bp.wpr; w0 += 256) {
        const int wx = w0 + tid;
        uint32_t c = 0;
        if (wx < bp.wpr) {
            const uint32_t cur = row[wx];
            if (cur) {
                uint32_t outer, hole;
                word_candidates(cur, wx > 0 ? row[wx - 1] >> 31 : 0u, wx + 1 < bp.wpr ? row[wx + 1] & 1u : 0u, wx, bp.w, outer, hole);
                c = __popc(outer) + __popc(hole);
            }
        }
        part[tid] = c;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {  // inclusive scan
            const uint32_t v = tid >= d ? part[tid - d] : 0u;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        if (wx < bp.wpr) pre[wx] = carry + part[tid] - c;
        __syncthreads();
        if (tid == 255) carry += part[255];
        __syncthreads();
    }
    if (tid == 0) rowcnt[t * bp.h + y] = carry;
}

// pass 2: first node of every row WITHIN its plane and the nodes per plane (one workgroup per plane), then the first
// node of every plane of the chunk (blob_bases_kernel; the host adds up the total).
__global__ __launch_bounds__(256) void blob_rowscan_kernel(int h, const uint32_t* rowcnt, uint32_t* rowoff, int* plane_cnt) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x, t = blockIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int y0 = 0; y0 < h; y0 += 256) {
        const int y = y0 + tid;
        const uint32_t c = y < h ? rowcnt[t * h + y] : 0u;
        part[tid] = c;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t v = tid >= d ? part[tid - d] : 0u;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        if (y < h) rowoff[t * h + y] = carry + part[tid] - c;
        __syncthreads();
        if (tid == 255) carry += part[255];
        __syncthreads();
    }
    if (tid == 0) plane_cnt[t] = (int)carry;
}
// exclusive prefix sums of n counts (wrap-around: the host checks the total before anything is indexed with them);
// workgroup b takes the pair (cnt_b, base_b): the planes' nodes, or the frames' records and points
__global__ __launch_bounds__(256) void blob_bases_kernel(const int* cnt0, int* base0, const int* cnt1, int* base1, int n) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x;
    const int* cnt = blockIdx.x ? cnt1 : cnt0;
    int* base = blockIdx.x ? base1 : base0;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const uint32_t c = i < n ? (uint32_t)cnt[i] : 0u;
        part[tid] = c;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t v = tid >= d ? part[tid - d] : 0u;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        if (i < n) base[i] = (int)(carry + part[tid] - c);
        __syncthreads();
        if (tid == 255) carry += part[255];
        __syncthreads();
    }
}

// node of candidate (x, type) of row y of plane t; `r1` = the row as 34 bits around word x >> 5 (row34)
__device__ __forceinline__ uint32_t node_of(const BitPlanes& bp, int t, int x, int y, int type, unsigned long long r1,
                                            const uint32_t* wordpre, const uint32_t* rowoff, uint32_t plane_base) {
    const int wx = x >> 5, b = x & 31;
    uint32_t outer, hole;
    word_candidates((uint32_t)(r1 >> 1), (uint32_t)(r1 & 1ull), (uint32_t)(r1 >> 33) & 1u, wx, bp.w, outer, hole);
    const uint32_t below = (1u << b) - 1u;
    return plane_base + rowoff[t * bp.h + y] + wordpre[((long long)t * bp.h + y) * bp.wpr + wx] + __popc(outer & below) +
           __popc(hole & below) + (type ? (outer >> b) & 1u : 0u);
}

// pass 3: the keys and the plane ids of the nodes, in place (thread per word)
__global__ __launch_bounds__(256) void blob_keys_kernel(BitPlanes bp, const uint32_t* wordpre, const uint32_t* rowoff, uint32_t* key,
                                                        uint16_t* plane, const int* plane_base) {
    const int wx = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, t = blockIdx.z;
    if (wx >= bp.wpr) return;
    const uint32_t* row = bp.bits + ((long long)t * bp.h + y) * bp.wpr;
    const uint32_t cur = row[wx];
    if (cur == 0) return;
    uint32_t outer, hole;
    word_candidates(cur, wx > 0 ? row[wx - 1] >> 31 : 0u, wx + 1 < bp.wpr ? row[wx + 1] & 1u : 0u, wx, bp.w, outer, hole);
    uint32_t k = (uint32_t)plane_base[t] + rowoff[t * bp.h + y] + wordpre[((long long)t * bp.h + y) * bp.wpr + wx];
    uint32_t both = outer | hole;
    while (both) {
        const int i = __ffs(both) - 1;
        both &= both - 1;
        const uint32_t xy = ((uint32_t)y << 16) | ((uint32_t)(wx * 32 + i) << 1);
        if ((outer >> i) & 1u) { plane[k] = (uint16_t)t; key[k++] = xy; }
        if ((hole >> i) & 1u) { plane[k] = (uint16_t)t; key[k++] = xy | 1u; }
    }
}

// The arc that starts at candidate `key` of plane t.  WRITE = false: -> (next node, steps, a00 share); a dead node
// (a single pixel, or the hole-type twin of an outer-type candidate in the same state) has 0 steps and is its own
// successor.  WRITE = true: stores the arc's points ((y << 16) | x) to pts[0 .. steps) and adds the arc's share of the
// other five contourMoments sums (a10, a01, a20, a11, a02: wrap-around integers like a00) to sums[0 .. 5).
template <bool WRITE>
__device__ __forceinline__ void blob_arc(const BitPlanes& bp, int t, uint32_t key, uint32_t self, const uint32_t* wordpre,
                                         const uint32_t* rowoff, uint32_t plane_base, uint32_t& next, uint32_t& steps,
                                         unsigned long long& a00, uint32_t* pts, unsigned long long* sums, int* err) {
    const int x0 = (int)((key >> 1) & 0x7fffu), y0 = (int)(key >> 16), is_hole = (int)(key & 1u);
    next = self;
    steps = 0;
    a00 = 0;
    BlobWin wn;
    wn.wx = -2;
    wn.y = -2;
    win_goto(wn, bp, t, x0, y0);
    uint32_t m = win_neighbours(wn, x0);
    int s = first_cw(m, is_hole ? 0 : 4);  // the predecessor of the start on the border
    if (s < 0) return;                     // a single pixel: area 0, never a blob
    if (is_hole && !(m & 0x10u) && first_cw(m, 4) == s) return;  // the outer-type candidate of this pixel is this state
    int x3 = x0, y3 = y0;
    uint32_t n = 0;
    constexpr unsigned long long kMask34 = (1ull << 34) - 1ull;
    for (;;) {
        const int from = s;
        s = first_ccw(m, s);  // the next border point
        // A straight horizontal run in one go.  Having come from the west and going east means that the three pixels
        // below were looked at first and are black, and the walk goes on east for as long as that stays so and the pixel
        // ahead is white (likewise westwards under a black row above): no candidate state on the way -- the pixel behind
        // is white (no outer-type start) and so is the one ahead (no hole-type start).  The run is read off the window's
        // rows with bit operations, up to the window's edge (32 steps); without this an arc along the frame's edge is
        // thousands of dependent iterations of ~150 instructions in one lane, and the launch lasts as long as that lane.
        int k = 1;
        const int b = x3 & 31;
        if (s == 0 && from == 4) {
            const unsigned long long dn = ~wn.r[2] & kMask34;
            const unsigned long long ok = dn & (dn >> 1) & (dn >> 2) & (wn.r[1] >> 2);  // bit b + j: step j of the run is possible
            k = __ffsll((long long)~(ok >> b)) - 1;
        } else if (s == 4 && from == 0) {
            const unsigned long long up = ~wn.r[0] & kMask34;
            const unsigned long long ok = up & (up >> 1) & (up >> 2) & wn.r[1];         // bit b - j
            k = __clzll((long long)~(ok << (63 - b)));
        }
        const int x4 = x3 + k * kDX[s], y4 = y3 + kDY[s];
        if (WRITE) {
            for (int j = 0; j < k; ++j) {  // the pair (point -> next point) of every step, as moments.cpp's contourMoments adds it
                const long long xa = x3 + j * kDX[s], ya = y3, xb = xa + kDX[s], yb = y4;  // (a run is horizontal: y4 == y3)
                pts[n + j] = ((uint32_t)y3 << 16) | (uint32_t)xa;
                const long long dxy = xa * yb - xb * ya, xii = xa + xb, yii = ya + yb;
                sums[0] += (unsigned long long)(dxy * xii);
                sums[1] += (unsigned long long)(dxy * yii);
                sums[2] += (unsigned long long)(dxy * (xa * xii + xb * xb));
                sums[3] += (unsigned long long)(dxy * (xa * (yii + ya) + xb * (yii + yb)));
                sums[4] += (unsigned long long)(dxy * (ya * yii + yb * yb));
            }
        } else {
            // contourMoments, the pairs (point -> next point) of the k steps: x * y' - x' * y each; in a horizontal run - y or + y
            a00 += k == 1 ? (unsigned long long)((long long)x3 * y4 - (long long)x4 * y3)
                          : (unsigned long long)((long long)k * (s == 0 ? -(long long)y3 : (long long)y3));
        }
        n += (uint32_t)k;
        // now at (x4, y4), having come from direction s + 4
        x3 = x4;
        y3 = y4;
        s = (s + 4) & 7;
        win_goto(wn, bp, t, x3, y3);
        m = win_neighbours(wn, x3);
        const bool outer_c = !(m & 0x10u) && first_cw(m, 4) == s;
        const bool hole_c = !(m & 1u) && first_cw(m, 0) == s;  // (the last column too: pseudo_node)
        if (outer_c || hole_c) {  // a candidate's start state (possibly this arc's own: a border of one arc)
            if (!WRITE) next = node_of(bp, t, x3, y3, outer_c ? 0 : 1, wn.r[1], wordpre, rowoff, plane_base);
            break;
        }
        if (n >= (uint32_t)kMaxArc) {
            if (!WRITE) atomicOr(err, 1);
            break;
        }
    }
    steps = n;
}

// pass 4: every arc (N = the nodes of the chunk, as the host added them up)
__global__ __launch_bounds__(256) void blob_arcs_kernel(BitPlanes bp, const uint32_t* wordpre, const uint32_t* rowoff, BlobNodes nd,
                                                        uint32_t N, BlobCounters cn) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    uint32_t next, steps;
    unsigned long long a00;
    const int t = nd.plane[i];
    blob_arc<false>(bp, t, nd.key[i], i, wordpre, rowoff, (uint32_t)cn.plane_base[t], next, steps, a00, nullptr, nullptr,
                    cn.err + t / kNumThresh);
    nd.next[i] = next;
    nd.n[i] = steps;
    nd.a00[i] = a00;
    nd.jmp[i] = next;
    nd.leader[i] = pseudo_node(nd.key[i], bp.w) ? kNoNode : i;
}

// pass 5, R rounds: the smallest node of every cycle.  Double-buffered ((jmp, leader) <-> the two list-ranking
// pointer arrays, which are free until pass 6): a round must see a node's minimum and its pointer from the SAME round,
// or the minimum it takes over may not cover the stretch the pointer skips.
__global__ __launch_bounds__(256) void blob_leader_round_kernel(const uint32_t* jmp, const uint32_t* lead, uint32_t* jmp_out,
                                                                uint32_t* lead_out, uint32_t N) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const uint32_t j = jmp[i];
    lead_out[i] = min(lead[i], lead[j]);
    jmp_out[i] = jmp[j];
}

// pass 6: the cycle cut open at its owner, then R rounds of list ranking (suffix sums towards the end of the list)
__global__ __launch_bounds__(256) void blob_rank_init_kernel(BlobNodes nd, uint32_t N) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const uint32_t nx = nd.next[i];
    nd.ptr[0][i] = nx == nd.leader[i] ? kNoNode : nx;
    nd.sa[0][i] = nd.a00[i];
    nd.sn[0][i] = nd.n[i];
    nd.off[i] = -1;
}
__global__ __launch_bounds__(256) void blob_rank_round_kernel(BlobNodes nd, int from, uint32_t N) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const int to = from ^ 1;
    const uint32_t p = nd.ptr[from][i];
    unsigned long long a = nd.sa[from][i];
    uint32_t n = nd.sn[from][i], q = kNoNode;
    if (p != kNoNode) {
        a += nd.sa[from][p];
        n += nd.sn[from][p];
        q = nd.ptr[from][p];
    }
    nd.ptr[to][i] = q;
    nd.sa[to][i] = a;
    nd.sn[to][i] = n;
}

struct BlobContour {      // one border that passed the area filter
    uint32_t key;         // its start (raster position and type): the order of discovery
    int32_t t;            // on the device: the plane within the chunk; on the host (blob_chunk_host): the threshold index
    int32_t n;            // points
    uint32_t points_off;  // first point in the chunk's arena
    long long a00, a10, a01, a20, a11, a02;  // contourMoments sums: a00 from the list ranking, the rest from the re-walk of the arcs
    int32_t pix;          // the frame's pixel at the rounded centre (filterByColor); -1: no centre, or one outside the frame
    int32_t pad;
};

// pass 7: the owners: filterByArea on m00 = |a00| / 2 (minArea 20 <= m00 < maxArea 80000, exact in integers).
// WRITE = false: how many contours of every frame pass and how many points they have -- the host sizes the record
// and point arrays from that, blob_bases_kernel gives every frame its stretch of both; WRITE = true: a record and a
// place in the point arena for each of them.
template <bool WRITE>
__global__ __launch_bounds__(256) void blob_records_kernel(BlobNodes nd, int rk, BlobContour* recs, uint32_t N, BlobCounters cn) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N || nd.leader[i] != i || nd.n[i] == 0) return;
    const long long a00 = (long long)nd.sa[rk][i];
    const long long a = a00 < 0 ? -a00 : a00;
    if (a < 2 * 20 || a >= 2 * 80000) return;
    const int n = (int)nd.sn[rk][i];
    const int plane = nd.plane[i], f = plane / kNumThresh;
    if (!WRITE) {
        atomicAdd(cn.rec_cnt + f, 1);
        atomicAdd(cn.pts_cnt + f, n);
        return;
    }
    BlobContour c;
    c.key = nd.key[i];
    c.t = plane;
    c.n = n;
    c.a00 = a00;
    c.a10 = c.a01 = c.a20 = c.a11 = c.a02 = 0;
    c.pix = -1;
    c.pad = 0;
    const uint32_t r = (uint32_t)cn.rec_base[f] + (uint32_t)atomicAdd(cn.rec_cur + f, 1);
    c.points_off = (uint32_t)cn.pts_base[f] + (uint32_t)atomicAdd(cn.pts_cur + f, n);
    nd.off[i] = (int)c.points_off;
    nd.jmp[i] = r;
    recs[r] = c;
}

// pass 8: the points of the contours that passed, every arc its own stretch: the arc's offset in its contour is
// what precedes it in the list from the owner = total - (points from this arc to the end).  The re-walk also yields the
// arc's share of the five moment sums the list ranking does not carry: exact and order-independent, so every arc adds
// its own to the contour's record.
__global__ __launch_bounds__(256) void blob_points_kernel(BitPlanes bp, const uint32_t* wordpre, const uint32_t* rowoff, BlobNodes nd,
                                                          int rk, uint32_t* pts, BlobContour* recs, uint32_t N) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N || nd.n[i] == 0) return;
    const uint32_t L = nd.leader[i];
    if (L == kNoNode) return;  // (every border has an outer-type start, so this cannot be: a guard for the index below)
    const int off = nd.off[L];
    if (off < 0) return;
    const uint32_t total = nd.sn[rk][L], at = total - nd.sn[rk][i];
    uint32_t next, steps;
    unsigned long long a00, sums[5] = {0, 0, 0, 0, 0};
    blob_arc<true>(bp, nd.plane[i], nd.key[i], i, wordpre, rowoff, 0u, next, steps, a00, pts + (uint32_t)off + at, sums, nullptr);
    unsigned long long* dst = (unsigned long long*)&recs[nd.jmp[L]].a10;
#pragma unroll
    for (int k = 0; k < 5; ++k) atomicAdd(dst + k, sums[k]);
}

// pass 9: filterByColor needs the frame's pixel at the rounded centre of every contour: the centre with the SAME IEEE
// double operations, in the same order, as contour_to_center below (the library is built with -ffp-contract=off for
// host and device; only *, / and round-to-nearest-even are used), then one pixel fetched.  Everything else about the
// contour stays on the host.
__global__ __launch_bounds__(256) void blob_colour_kernel(BlobContour* recs, int nrecs, const uint8_t* img, long long frame_pitch,
                                                          int stride, int w, int h) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrecs) return;
    const BlobContour c = recs[r];
    const double a00 = (double)c.a00, a10 = (double)c.a10, a01 = (double)c.a01;
    const double sg = a00 > 0 ? 1.0 : -1.0;
    const double m00 = a00 * (sg * 0.5), m10 = a10 * (sg * 0.16666666666666666666666666666667);
    const double m01 = a01 * (sg * 0.16666666666666666666666666666667);
    int pix = -1;
    if (m00 != 0.0) {
        const double x = rint(m10 / m00), y = rint(m01 / m00);  // cvRound
        if (x >= 0. && x < (double)w && y >= 0. && y < (double)h)
            pix = img[(c.t / kNumThresh) * frame_pitch + (long long)(int)y * stride + (int)x];
    }
    recs[r].pix = pix;
}

// ---------------------------------------------------------------------------------------------
// host: the double-precision part of SimpleBlobDetector::findBlobs and the grouping of detect()
// ---------------------------------------------------------------------------------------------
struct Center { double x, y, radius, confidence; };

struct IPt { int x, y; };

double polygon_area(const IPt* p, int n) {  // cv::contourArea, not oriented
    if (n == 0) return 0.;
    double a00 = 0, xp = p[n - 1].x, yp = p[n - 1].y;
    for (int i = 0; i < n; ++i) {
        const double x = p[i].x, y = p[i].y;
        a00 += xp * y - x * yp;
        xp = x;
        yp = y;
    }
    return std::fabs(a00 * 0.5);
}

double hull_area(std::vector<IPt> s) {  // area of the convex hull of the point set (monotone chain)
    const int n = (int)s.size();
    std::sort(s.begin(), s.end(), [](const IPt& a, const IPt& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
    auto cross = [](const IPt& o, const IPt& a, const IPt& b) {
        return (long long)(a.x - o.x) * (b.y - o.y) - (long long)(a.y - o.y) * (b.x - o.x);
    };
    std::vector<IPt> hull((size_t)2 * n + 2);
    int k = 0;
    for (int i = 0; i < n; ++i) {
        while (k >= 2 && cross(hull[k - 2], hull[k - 1], s[i]) <= 0) --k;
        hull[k++] = s[i];
    }
    for (int i = n - 2, t = k + 1; i >= 0; --i) {
        while (k >= t && cross(hull[k - 2], hull[k - 1], s[i]) <= 0) --k;
        hull[k++] = s[i];
    }
    return polygon_area(hull.data(), k > 1 ? k - 1 : k);
}

// blobdetector.cpp findBlobs for one contour that passed the area filter
bool contour_to_center(const BlobContour& c, const uint32_t* pts, Center* out) {
    // contourMoments: scale the sums, then completeMomentState
    const double a00 = (double)c.a00, a10 = (double)c.a10, a01 = (double)c.a01;
    const double a20 = (double)c.a20, a11 = (double)c.a11, a02 = (double)c.a02;
    if (!(std::fabs(a00) > FLT_EPSILON)) return false;
    const double sg = a00 > 0 ? 1.0 : -1.0;
    const double m00 = a00 * (sg * 0.5), m10 = a10 * (sg * 0.16666666666666666666666666666667);
    const double m01 = a01 * (sg * 0.16666666666666666666666666666667);
    const double m20 = a20 * (sg * 0.083333333333333333333333333333333);
    const double m11 = a11 * (sg * 0.041666666666666666666666666666667);
    const double m02 = a02 * (sg * 0.083333333333333333333333333333333);
    double cx = 0, cy = 0;
    if (std::fabs(m00) > DBL_EPSILON) {
        const double inv = 1. / m00;
        cx = m10 * inv;
        cy = m01 * inv;
    }
    const double mu20 = m20 - m10 * cx, mu11 = m11 - m10 * cy, mu02 = m02 - m01 * cy;
    if (m00 < 20. || m00 >= 80000.) return false;  // filterByArea (the device already applied it)
    double ratio;                                   // filterByInertia, minInertiaRatio 0.1
    const double denominator = std::sqrt((2 * mu11) * (2 * mu11) + (mu20 - mu02) * (mu20 - mu02));
    if (denominator > 1e-2) {
        const double cosmin = (mu20 - mu02) / denominator, sinmin = 2 * mu11 / denominator;
        const double cosmax = -cosmin, sinmax = -sinmin;
        const double imin = 0.5 * (mu20 + mu02) - 0.5 * (mu20 - mu02) * cosmin - mu11 * sinmin;
        const double imax = 0.5 * (mu20 + mu02) - 0.5 * (mu20 - mu02) * cosmax - mu11 * sinmax;
        ratio = imin / imax;
    } else {
        ratio = 1;
    }
    if (ratio < (double)0.1f || ratio >= FLT_MAX) return false;  // Params::minInertiaRatio is a float: 0.100000001490...
    if (m00 == 0.0) return false;
    out->x = m10 / m00;
    out->y = m01 / m00;
    out->confidence = ratio * ratio;
    {  // filterByColor, blobColor 0: the binarised pixel at the rounded centre must be dark.  (blobdetector.cpp checks it
       // after the convexity; the filters are independent conditions, and this one spares the contours of the WHITE
       // regions -- half of all -- their convex hull).  The pixel at (cvRound(x), cvRound(y)) comes from the device:
       // blob_colour_kernel
        if (c.pix < 0 || c.pix > kThresh0 + kThreshStep * c.t) return false;
    }
    std::vector<IPt> p((size_t)c.n);
    for (int i = 0; i < c.n; ++i) p[i] = IPt{(int)(pts[i] & 0xffffu), (int)(pts[i] >> 16)};
    {  // filterByConvexity, minConvexity 0.95
        const double carea = polygon_area(p.data(), c.n), harea = hull_area(p);
        if (std::fabs(harea) < DBL_EPSILON) return false;
        const double conv = carea / harea;
        if (conv < (double)0.95f || conv >= FLT_MAX) return false;  // Params::minConvexity is a float: 0.949999988079...
    }
    std::vector<double> d((size_t)c.n);
    for (int i = 0; i < c.n; ++i) {
        const double dx = out->x - p[i].x, dy = out->y - p[i].y;
        d[i] = std::sqrt(dx * dx + dy * dy);
    }
    // the two middle order statistics (blobdetector.cpp sorts the whole list; the values are the same)
    const size_t lo = (size_t)(c.n - 1) / 2, hi = (size_t)c.n / 2;
    std::nth_element(d.begin(), d.begin() + lo, d.end());
    const double dlo = d[lo];
    const double dhi = hi == lo ? dlo : *std::min_element(d.begin() + lo + 1, d.end());
    out->radius = (dlo + dhi) / 2.;
    return true;
}

}  // namespace


namespace {

// blobdetector.cpp detect() for one frame: the centres of one blob across thresholds grouped, the keypoints of the
// groups appended as (x, y) * 1000 ints.  rec[0 .. n): the frame's contours, threshold ascending.
void group_keypoints(const BlobContour* rec, const Center* centers, const char* keep, size_t n, std::vector<int32_t>& xy_out) {
    std::vector<std::vector<Center>> groups;
    size_t i = 0;
    for (int t = 0; t < kNumThresh; ++t) {
        std::vector<Center> cur;
        for (; i < n && rec[i].t == t; ++i)
            if (keep[i]) cur.push_back(centers[i]);
        std::vector<std::vector<Center>> fresh;
        for (const Center& c : cur) {
            bool is_new = true;
            for (auto& g : groups) {
                const Center& mid = g[g.size() / 2];
                const double dx = mid.x - c.x, dy = mid.y - c.y;
                const double dist = std::sqrt(dx * dx + dy * dy);
                is_new = dist >= 5. && dist >= mid.radius && dist >= c.radius;  // minDistBetweenBlobs 5
                if (!is_new) {
                    g.push_back(c);
                    size_t k = g.size() - 1;
                    while (k > 0 && c.radius < g[k - 1].radius) { g[k] = g[k - 1]; --k; }
                    g[k] = c;
                    break;
                }
            }
            if (is_new) fresh.push_back(std::vector<Center>(1, c));
        }
        for (auto& g : fresh) groups.push_back(std::move(g));
    }
    for (const auto& g : groups) {
        if (g.size() < 2) continue;  // minRepeatability 2
        double sx = 0, sy = 0, norm = 0;
        for (const Center& c : g) {
            sx += c.confidence * c.x;
            sy += c.confidence * c.y;
            norm += c.confidence;
        }
        const double inv = 1. / norm;
        sx *= inv;
        sy *= inv;
        const float fx = (float)sx, fy = (float)sy;        // KeyPoint::pt is a Point2f
        const float tx = fx * 1000.0f, ty = fy * 1000.0f;  // it->pt.x * FIND_GRID_SCALE, find_blobs.cc:40-41
        xy_out.push_back((int)((double)tx + 0.5));
        xy_out.push_back((int)((double)ty + 0.5));
    }
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// plane scratch of a chunk of nf frames: the counters, then bit planes, word prefixes, row counts and row offsets of
// its nf * 17 planes
struct ChunkLayout {
    int wpr;
    size_t o_counters, o_bits, o_wordpre, o_rowcnt, o_rowoff, bytes;
};
ChunkLayout chunk_layout(int w, int h, int nf) {
    ChunkLayout L;
    L.wpr = (w + 31) / 32;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t planes = (size_t)nf * kNumThresh;
    L.o_counters = take((size_t)blob_counter_words(nf) * sizeof(int));
    L.o_bits = take(planes * h * L.wpr * 4);
    L.o_wordpre = take(planes * h * L.wpr * 4);
    L.o_rowcnt = take(planes * h * 4);
    L.o_rowoff = take(planes * h * 4);
    L.bytes = off;
    return L;
}

constexpr int kBadNodes = 1, kBadArc = 2;  // why a frame has no result (blob_detect_batch)

// Frames [f0, f0 + nf) of the batch as ONE chunk: every kernel once, three round trips (node counts; record and point
// counts; records and points), the filters of all its contours on `nthreads` host threads, the grouping per frame.
// 0: xy[f0 ..] hold the keypoints (a lone frame with an arc above kMaxArc: bad[f0] = kBadArc instead); 1: more nodes or
// points than one node space takes, or an arc above kMaxArc somewhere in a chunk of several frames -- the caller
// splits the chunk; < 0: an error code.
int blob_chunk(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int f0, int nf, int nthreads, std::vector<int32_t>* xy,
               char* bad) {
    const int w = fr->width, h = fr->height, P = nf * kNumThresh, nwords = blob_counter_words(nf);
    const ChunkLayout L = chunk_layout(w, h, nf);
    int rc;
    if ((rc = ensure(ctx, ctx->blob_scratch, L.bytes))) return rc;
    hipStream_t s = ctx->pix;
    char* base = (char*)ctx->blob_scratch.p;
    int* words = (int*)(base + L.o_counters);
    auto counters_at = [&](int* p) {
        BlobCounters c;
        c.err = p;
        c.plane_cnt = c.err + nf;
        c.plane_base = c.plane_cnt + P;
        c.rec_cnt = c.plane_base + P;
        c.pts_cnt = c.rec_cnt + nf;
        c.rec_base = c.pts_cnt + nf;
        c.pts_base = c.rec_base + nf;
        c.rec_cur = c.pts_base + nf;
        c.pts_cur = c.rec_cur + nf;
        return c;
    };
    const BlobCounters cn = counters_at(words);
    std::vector<int> hwords((size_t)nwords);
    const BlobCounters hc = counters_at(hwords.data());
    uint32_t* bits = (uint32_t*)(base + L.o_bits);
    uint32_t* wordpre = (uint32_t*)(base + L.o_wordpre);
    uint32_t* rowcnt = (uint32_t*)(base + L.o_rowcnt);
    uint32_t* rowoff = (uint32_t*)(base + L.o_rowoff);
    const BitPlanes bp{bits, w, h, L.wpr};
    const uint8_t* img = fr->frames + (size_t)f0 * fr->frame_pitch;
    // device time of the chunk's kernels (kernel timing on): events around each of the three stretches of kernels
    const bool timed = ctx->timing;
    if (timed)
        for (Event& e : ctx->blob_ev) MRG_HIP_CHECK(e.create(hipEventDefault));
    auto kernels_begin = [&] { if (timed) hipEventRecord(ctx->blob_ev[0], s); };
    auto kernels_end = [&] { if (timed) hipEventRecord(ctx->blob_ev[1], s); };
    // the counters back on the host: one copy, one synchronisation
    auto round_trip = [&]() -> int {
        if (hipMemcpyAsync(hwords.data(), words, (size_t)nwords * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "blob detector: device error (%s)", hipGetErrorString(hipGetLastError()));
        float ms = 0.f;
        if (timed && hipEventElapsedTime(&ms, ctx->blob_ev[0], ctx->blob_ev[1]) == hipSuccess) ctx->blob_stat[5] += ms;
        return 0;
    };

    hipMemsetAsync(words, 0, (size_t)nwords * sizeof(int), s);
    kernels_begin();
    const dim3 grid_rows((L.wpr + 255) / 256, h, nf);
    hipLaunchKernelGGL(blob_bitplanes_kernel, grid_rows, dim3(256), 0, s, img, (long long)fr->frame_pitch, fr->stride, w, h, L.wpr, bits);
    hipLaunchKernelGGL(blob_count_kernel, dim3(h, P), dim3(256), 0, s, bp, wordpre, rowcnt);
    hipLaunchKernelGGL(blob_rowscan_kernel, dim3(P), dim3(256), 0, s, h, (const uint32_t*)rowcnt, rowoff, cn.plane_cnt);
    hipLaunchKernelGGL(blob_bases_kernel, dim3(1), dim3(256), 0, s, (const int*)cn.plane_cnt, cn.plane_base, (const int*)nullptr,
                       (int*)nullptr, P);
    kernels_end();
    if ((rc = round_trip())) return rc;
    long long N = 0;
    int maxn = 1;
    for (int p = 0; p < P; ++p) {
        N += hc.plane_cnt[p];
        maxn = std::max(maxn, hc.plane_cnt[p]);
    }
    if (N > (1ll << 27)) return 1;
    ctx->blob_stat[1] += 1;
    ctx->blob_stat[2] += (double)N;
    size_t R = 0, Np = 0;
    std::vector<BlobContour> hrec;
    std::vector<uint32_t> hpts;
    if (N > 0) {
        if ((rc = ensure(ctx, ctx->blob_nodes, (size_t)N * kBlobNodeBytes + 16 * 256))) return rc;
        char* nb = (char*)ctx->blob_nodes.p;
        BlobNodes nd;
        size_t off = 0;
        auto take = [&](size_t bytes) { char* p = nb + off; off += (bytes * (size_t)N + 255) / 256 * 256; return p; };
        nd.a00 = (unsigned long long*)take(8);
        nd.sa[0] = (unsigned long long*)take(8);
        nd.sa[1] = (unsigned long long*)take(8);
        nd.key = (uint32_t*)take(4);
        nd.next = (uint32_t*)take(4);
        nd.n = (uint32_t*)take(4);
        nd.jmp = (uint32_t*)take(4);
        nd.leader = (uint32_t*)take(4);
        nd.ptr[0] = (uint32_t*)take(4);
        nd.ptr[1] = (uint32_t*)take(4);
        nd.sn[0] = (uint32_t*)take(4);
        nd.sn[1] = (uint32_t*)take(4);
        nd.off = (int32_t*)take(4);
        nd.plane = (uint16_t*)take(2);
        int rounds = 1;  // 2^rounds >= the longest cycle (in arcs) there can be: the largest plane of the chunk
        while ((1ll << rounds) < maxn) ++rounds;
        const uint32_t n32 = (uint32_t)N;
        const dim3 gn((unsigned)((N + 255) / 256));
        kernels_begin();
        hipLaunchKernelGGL(blob_keys_kernel, dim3(grid_rows.x, h, P), dim3(256), 0, s, bp, (const uint32_t*)wordpre,
                           (const uint32_t*)rowoff, nd.key, nd.plane, (const int*)cn.plane_base);
        hipLaunchKernelGGL(blob_arcs_kernel, gn, dim3(256), 0, s, bp, (const uint32_t*)wordpre, (const uint32_t*)rowoff, nd, n32, cn);
        for (int r = 0; r < (rounds + 1) / 2 * 2; ++r)  // (an even number: the result is back in (jmp, leader))
            if (r & 1)
                hipLaunchKernelGGL(blob_leader_round_kernel, gn, dim3(256), 0, s, (const uint32_t*)nd.ptr[0], (const uint32_t*)nd.ptr[1],
                                   nd.jmp, nd.leader, n32);
            else
                hipLaunchKernelGGL(blob_leader_round_kernel, gn, dim3(256), 0, s, (const uint32_t*)nd.jmp, (const uint32_t*)nd.leader,
                                   nd.ptr[0], nd.ptr[1], n32);
        hipLaunchKernelGGL(blob_rank_init_kernel, gn, dim3(256), 0, s, nd, n32);
        int rk = 0;
        for (int r = 0; r < rounds; ++r, rk ^= 1) hipLaunchKernelGGL(blob_rank_round_kernel, gn, dim3(256), 0, s, nd, rk, n32);
        // how many contours of every frame pass the area filter, and how many points they have: the arrays for them are
        // sized from that, and every frame gets its own stretch of both
        hipLaunchKernelGGL(blob_records_kernel<false>, gn, dim3(256), 0, s, nd, rk, (BlobContour*)nullptr, n32, cn);
        hipLaunchKernelGGL(blob_bases_kernel, dim3(2), dim3(256), 0, s, (const int*)cn.rec_cnt, cn.rec_base, (const int*)cn.pts_cnt,
                           cn.pts_base, nf);
        kernels_end();
        if ((rc = round_trip())) return rc;
        for (int f = 0; f < nf; ++f)
            if (hc.err[f]) {  // (its lists are cut: nothing of the chunk's record counts can be trusted)
                if (nf > 1) return 1;
                bad[f0] = kBadArc;
                return 0;
            }
        for (int f = 0; f < nf; ++f) {
            R += (size_t)(uint32_t)hc.rec_cnt[f];
            Np += (size_t)(uint32_t)hc.pts_cnt[f];
        }
        if (Np > 0x7fffffffull) return 1;  // (point offsets are 31 bits)
        if (R > 0) {
            const size_t rec_bytes = (R * sizeof(BlobContour) + 255) / 256 * 256;
            if ((rc = ensure(ctx, ctx->blob_out, rec_bytes + Np * 4))) return rc;
            BlobContour* recs = (BlobContour*)ctx->blob_out.p;
            uint32_t* pts = (uint32_t*)((char*)ctx->blob_out.p + rec_bytes);
            kernels_begin();
            hipLaunchKernelGGL(blob_records_kernel<true>, gn, dim3(256), 0, s, nd, rk, recs, n32, cn);
            hipLaunchKernelGGL(blob_points_kernel, gn, dim3(256), 0, s, bp, (const uint32_t*)wordpre, (const uint32_t*)rowoff, nd, rk,
                               pts, recs, n32);
            hipLaunchKernelGGL(blob_colour_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, recs, (int)R, img,
                               (long long)fr->frame_pitch, fr->stride, w, h);
            kernels_end();
            hrec.resize(R);
            hpts.resize(Np);
            if (hipMemcpyAsync(hrec.data(), recs, R * sizeof(BlobContour), hipMemcpyDeviceToHost, s) != hipSuccess ||
                (Np && hipMemcpyAsync(hpts.data(), pts, Np * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
                hipStreamSynchronize(s) != hipSuccess)
                return fail(ctx, MRGINGHAM_AMD_ERR_DEVICE, "blob detector: download failed (%s)", hipGetErrorString(hipGetLastError()));
            float ms = 0.f;
            if (timed && hipEventElapsedTime(&ms, ctx->blob_ev[0], ctx->blob_ev[1]) == hipSuccess) ctx->blob_stat[5] += ms;
        }
    }
    ctx->blob_stat[3] += (double)R;
    ctx->blob_stat[4] += (double)Np;

    // host: per frame its contours in cv::findContours' RETR_LIST order per threshold (discovery order = raster order of the
    // starts, reversed); the per-contour filters (moments, hull, radius: independent, ~40 ns per contour point) of the
    // whole chunk; the grouping per frame
    const double t_host = now_ms();
    std::vector<size_t> first((size_t)nf + 1, 0);
    for (int f = 0; f < nf; ++f) first[f + 1] = first[f] + (size_t)(uint32_t)hc.rec_cnt[f];
    std::vector<Center> centers(R);
    std::vector<char> keep(R, 0);
    constexpr size_t kBlock = 32;  // contours a thread takes at a time
    std::atomic<size_t> next_sort{0}, next_block{0}, next_group{0};
    auto sort_frames = [&] {
        for (size_t f; (f = next_sort.fetch_add(1)) < (size_t)nf;) {
            for (size_t k = first[f]; k < first[f + 1]; ++k) hrec[k].t %= kNumThresh;
            std::sort(hrec.begin() + first[f], hrec.begin() + first[f + 1],
                      [](const BlobContour& a, const BlobContour& b) { return a.t != b.t ? a.t < b.t : a.key > b.key; });
        }
    };
    auto filter_blocks = [&] {
        for (size_t b; (b = next_block.fetch_add(1)) * kBlock < R;)
            for (size_t k = b * kBlock; k < std::min(R, (b + 1) * kBlock); ++k)
                keep[k] = contour_to_center(hrec[k], hpts.data() + hrec[k].points_off, &centers[k]);
    };
    auto group_frames = [&] {
        for (size_t f; (f = next_group.fetch_add(1)) < (size_t)nf;)
            group_keypoints(hrec.data() + first[f], centers.data() + first[f], keep.data() + first[f], first[f + 1] - first[f], xy[f0 + f]);
    };
    const int nthr = (int)std::min<size_t>((size_t)nthreads, Np / 16384 + 1);
    ctx->pool.run(std::min(nthr, nf), sort_frames);
    ctx->pool.run(nthr, filter_blocks);
    ctx->pool.run(std::min(nthr, nf), group_frames);
    ctx->blob_stat[6] += now_ms() - t_host;
    return 0;
}

// chunk [f0, f0 + nf), halved for as long as it does not fit one node space; a lone frame that does not is left out
int blob_chunk_split(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int f0, int nf, int nthreads, std::vector<int32_t>* xy,
                     char* bad) {
    const int rc = blob_chunk(ctx, fr, f0, nf, nthreads, xy, bad);
    if (rc != 1) return rc;
    if (nf == 1) {
        bad[f0] = kBadNodes;
        return 0;
    }
    const int half = nf / 2;
    const int ra = blob_chunk_split(ctx, fr, f0, half, nthreads, xy, bad);
    return ra ? ra : blob_chunk_split(ctx, fr, f0 + half, nf - half, nthreads, xy, bad);
}

}  // namespace

// find_blobs_from_image_array (find_blobs.cc:14-46) for every frame of a batch on the context's device: xy[f] receives
// frame f's keypoints as (x, y) * 1000 ints in SimpleBlobDetector's output order.  The batch is worked through in chunks
// of frames whose plane scratch stays within ctx->blob_plane_budget (option "blob_chunk_frames": at most that many frames).
// Returns 0; MRGINGHAM_AMD_ERR_CAPACITY when a frame has more border starts than a node space takes (2^27) or an arc above
// 2^20 steps -- bad[f] != 0 for such a frame, the others are delivered --; another error code when the device fails.
// Synchronous; the sizes have been checked by the caller (sides up to 32767 x 65535).
int blob_detect_batch(mrgingham_amd_ctx* ctx, const mrgingham_amd_frames* fr, int nthreads, std::vector<std::vector<int32_t>>& xy,
                      std::vector<char>& bad) {
    const int B = fr->nframes;
    xy.assign((size_t)B, std::vector<int32_t>());
    bad.assign((size_t)B, 0);
    if (B <= 0 || fr->width <= 0 || fr->height <= 0) return 0;
    fb_drain(ctx);  // (their grid finder runs on the pool the filters use)
    const size_t per_frame = chunk_layout(fr->width, fr->height, 1).bytes;
    int chunk = (int)std::min<size_t>(std::max<size_t>(ctx->blob_plane_budget / per_frame, 1), (size_t)kMaxChunkFrames);
    if (ctx->blob_chunk_frames > 0) chunk = std::min(chunk, ctx->blob_chunk_frames);
    ctx->blob_stat[0] += 1;
    ctx->blob_stat[7] += B;
    for (int f0 = 0; f0 < B; f0 += chunk) {
        const int rc = blob_chunk_split(ctx, fr, f0, std::min(chunk, B - f0), nthreads, xy.data(), bad.data());
        if (rc) return rc;
    }
    for (int f = 0; f < B; ++f)
        if (bad[f])
            return fail(ctx, MRGINGHAM_AMD_ERR_CAPACITY, "%s",
                        bad[f] == kBadArc ? "blob detector: a border arc longer than 2^20 steps"
                                          : "blob detector: more border starts than it takes (pure noise?)");
    return 0;
}

}  // namespace mrg
