// The CLI's 16-bit branch (mrgingham-from-image.cc:85-92, then the box blur of :106-111) for a BATCH of frames on the
// device: bit for bit what launch_preprocess16 + launch_box_blur compute (and oracle_preprocess16), in three passes over
// the pixels instead of seven kernels, and without the 16-bit normalised copy of the frame.  The 8-bit path's design
// (preprocess.hip) carried over to 16 bits:
//   extrema          2 B/px read      one reduction per frame
//   tile histograms  2 B/px read      RAW values over the frame's occupied range [smin, smax] (R = smax - smin + 1
//                                     bins) in LDS: slabs of 16-bit counters while R <= 4 096, else whole tiles in
//                                     parts of 16 384 32-bit counters (the tile re-read per part, from the caches)
//   tile tables      R bins per tile  cv::normalize's value map applied to the BINS, clip + redistribution + cumulative
//                                     LUT over the occupied bins only, composed with the value map: lut[tile][v - smin]
//   blend + blur     2 B/px read      bilinear blend of the four tile tables (OpenCV's single-precision expression,
//                    1 B/px written   rounded to u16, then convertTo(CV_8U)), the 3x3 box blur of that in the same pass
// do_clahe = 0 is the last pass alone (convertTo + blur).  Blur radii other than 1 go through an 8-bit intermediate and
// launch_box_blur.
#include "common.h"
#include "kernels.h"
#include "pre16.h"

namespace mrg {

namespace {

using namespace pre16;

constexpr int kTileCount = kTiles16 * kTiles16;
constexpr long long kTableEntries = (long long)kTileCount * kBins16;  // per frame: tables are laid out for R = 65 536
constexpr int kLdsSmallBins = 4096, kLdsSmallCopies = 4;              // the small range class (p16_hist_small_kernel)
constexpr int kSlabPixels = 65535;  // pixels of a histogram workgroup's slab: a 16-bit LDS counter cannot overflow
using u32x4n = uint32_t __attribute__((ext_vector_type(4)));

// the frame extrema: mm[2 f] = smin, mm[2 f + 1] = ~smax (both start at 0xffffffff: one memset, atomicMin for both)
__device__ __forceinline__ void frame_range(const unsigned* mm, int f, unsigned& smin, unsigned& smax) {
    smin = mm[2 * f];
    smax = ~mm[2 * f + 1];
}

struct Frames16 {
    const uint16_t* frames;
    long long pitch;  // elements between frames
    int w, h, stride;  // stride in elements
    bool vec;          // rows of whole, 16-byte aligned groups of 8 pixels
};

// grid (ceil(h / 16), nframes): 16 rows per workgroup, one pair of atomics per workgroup
__global__ __launch_bounds__(256) void p16_minmax_kernel(Frames16 in, unsigned* mm) {
    __shared__ unsigned red[8];
    const int f = blockIdx.y, tid = threadIdx.x;
    const uint16_t* img = in.frames + (long long)f * in.pitch;
    const int y0 = blockIdx.x * 16, y1 = min(y0 + 16, in.h);
    unsigned lo = 0xffffu, hi = 0u;
    if (in.vec) {
        const int chunks = in.w / 8, n = (y1 - y0) * chunks;
        for (int i = tid; i < n; i += 256) {
            const int r = i / chunks, c = i - r * chunks;
            const u32x4n q = __builtin_nontemporal_load(
                reinterpret_cast<const u32x4n*>(img + (long long)(y0 + r) * in.stride + 8 * c));
            const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo = min(lo, min(qq[k] & 0xffffu, qq[k] >> 16));
                hi = max(hi, max(qq[k] & 0xffffu, qq[k] >> 16));
            }
        }
    } else {
        for (int y = y0; y < y1; ++y)
            for (int x = tid; x < in.w; x += 256) {
                const unsigned v = img[(long long)y * in.stride + x];
                lo = min(lo, v);
                hi = max(hi, v);
            }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o));
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = lo;
        red[4 + (tid >> 6)] = hi;
    }
    __syncthreads();
    if (tid == 0) {
        atomicMin(mm + 2 * f, min(min(red[0], red[1]), min(red[2], red[3])));
        atomicMin(mm + 2 * f + 1, ~max(max(red[4], red[5]), max(red[6], red[7])));
    }
}

// grid (64 tiles, nframes): the global tile histograms of a frame of the small class (64 x R words) to zero; the other
// frames' histograms are stored whole by p16_hist_parts_kernel
__global__ __launch_bounds__(256) void p16_zero_kernel(const unsigned* mm, unsigned* hist) {
    const int f = blockIdx.y, tile = blockIdx.x;
    unsigned smin, smax;
    frame_range(mm, f, smin, smax);
    const int R = (int)(smax - smin) + 1;
    if (R > kLdsSmallBins) return;
    unsigned* hh = hist + (long long)f * kTableEntries + (long long)tile * R;
    for (int i = threadIdx.x; i < R; i += 256) hh[i] = 0;
}

// every pixel of rows [y0, y1) x columns [x0, x0 + tw) of the REFLECT_101-extended frame, dealt to the 256 threads: 16-byte
// loads where the frame is not padded and its rows are aligned
template <typename F>
__device__ __forceinline__ void for_pixels(const Frames16& in, const Geom16& g, const uint16_t* img, int y0, int y1, int x0, F&& count) {
    const int tid = threadIdx.x;
    if (in.vec && g.ew == in.w && g.eh == in.h && g.tw % 8 == 0) {
        const int chunks = g.tw / 8, n = (y1 - y0) * chunks;
        const uint16_t* base = img + (long long)y0 * in.stride + x0;
        for (int i = tid; i < n; i += 256) {
            const int r = i / chunks, c = i - r * chunks;
            const u32x4n q = __builtin_nontemporal_load(reinterpret_cast<const u32x4n*>(base + (long long)r * in.stride + 8 * c));
            const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                count(qq[k] & 0xffffu);
                count(qq[k] >> 16);
            }
        }
    } else {
        const long long n = (long long)(y1 - y0) * g.tw;
        for (long long i = tid; i < n; i += 256) {
            const int r = (int)(i / g.tw), c = (int)(i - (long long)r * g.tw);
            const int y = reflect101_16(y0 + r, in.h), x = reflect101_16(x0 + c, in.w);
            count(img[(long long)y * in.stride + x]);
        }
    }
}

// The raw-value tile histograms, counted relative to the frame's minimum, by the frame's range R = smax - smin + 1.
// Small class, R <= 4 096 (12-bit sources): grid (slabs, 64 tiles, nframes), a workgroup counts a slab of one tile (at most
// kSlabPixels pixels) into kLdsSmallCopies interleaved LDS histograms (copy = lane % copies: lanes on one value of a flat
// region meet fewer of each other) of 16-bit counters, two to a word (bin 2j in the low half of word j): a slab has at
// most 65 535 pixels, so a half never carries into its neighbour.  32 KiB of LDS; the sums are added to the frame's
// (zeroed) global table with one atomic per occupied bin.
__global__ __launch_bounds__(256) void p16_hist_small_kernel(Frames16 in, Geom16 g, const unsigned* mm, unsigned* hist, int rows_per_slab) {
    constexpr int C = kLdsSmallCopies;
    __shared__ uint32_t lh[kLdsSmallBins / 2 * C];  // [bin / 2][copy]
    const int f = blockIdx.z, tile = blockIdx.y, ty = tile / kTiles16, tx = tile % kTiles16, tid = threadIdx.x;
    unsigned smin, smax;
    frame_range(mm, f, smin, smax);
    const int R = (int)(smax - smin) + 1;
    if (R > kLdsSmallBins) return;  // p16_hist_parts_kernel takes this frame
    for (int i = tid; i < (R + 1) / 2 * C; i += 256) lh[i] = 0;
    __syncthreads();
    const int copy = tid & (C - 1);
    const int y0 = ty * g.th + blockIdx.x * rows_per_slab, y1 = min(y0 + rows_per_slab, (ty + 1) * g.th);
    for_pixels(in, g, in.frames + (long long)f * in.pitch, y0, y1, tx * g.tw, [&](unsigned v) {
        const unsigned i = v - smin;
        atomicAdd(&lh[(i >> 1) * C + copy], 1u << (16 * (i & 1)));
    });
    __syncthreads();
    unsigned* hh = hist + (long long)f * kTableEntries + (long long)tile * R;
    for (int i = tid; i < R; i += 256) {
        unsigned total = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) total += (lh[(i >> 1) * C + c] >> (16 * (i & 1))) & 0xffffu;
        if (total) __hip_atomic_fetch_add(hh + i, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Larger ranges: grid (kMaxParts, 64 tiles, nframes), workgroup (part, tile) counts the values [part, part + 1) x
// kPartBins above smin of the WHOLE tile in 32-bit LDS counters (64 KiB; one bin of a 4096x3072 tile can hold all its
// 196 608 pixels) and stores them: no global atomics, no zeroing.  The tile is read ceil(R / kPartBins) times -- up to
// 8 B/px for full-range data, from HBM once and from the L2 / MALL after that, in place of a random device-scope atomic
// per pixel (64 full-range frames of 4096x3072, clahe + blur 1: 34.9 ms per batch, 62.0 ms with the atomics; this kernel
// is 2.5 ms of the 34.9).
constexpr int kPartBins = 16384, kMaxParts = kBins16 / kPartBins;
__global__ __launch_bounds__(256) void p16_hist_parts_kernel(Frames16 in, Geom16 g, const unsigned* mm, unsigned* hist) {
    __shared__ uint32_t lh[kPartBins];
    const int f = blockIdx.z, tile = blockIdx.y, ty = tile / kTiles16, tx = tile % kTiles16, tid = threadIdx.x;
    unsigned smin, smax;
    frame_range(mm, f, smin, smax);
    const int R = (int)(smax - smin) + 1, lo = blockIdx.x * kPartBins;
    if (R <= kLdsSmallBins || lo >= R) return;
    const int nb = min(R - lo, kPartBins);
    for (int i = tid; i < nb; i += 256) lh[i] = 0;
    __syncthreads();
    const unsigned base = smin + lo;
    for_pixels(in, g, in.frames + (long long)f * in.pitch, ty * g.th, (ty + 1) * g.th, tx * g.tw, [&](unsigned v) {
        const unsigned i = v - base;
        if (i < (unsigned)nb) atomicAdd(&lh[i], 1u);
    });
    __syncthreads();
    unsigned* hh = hist + (long long)f * kTableEntries + (long long)tile * R + lo;
    for (int i = tid; i < nb; i += 256) hh[i] = lh[i];
}

// grid (64 tiles, nframes), 256 threads: the tile's composed table lut[v - smin] = LUT(n(v)), n = cv::normalize's value map.
// n is monotone but not always injective (float rounding): raw bins whose n is equal are ONE bin of the normalised
// histogram, merged before clipping.  Thread t owns the whole runs of equal n that start in [t per, (t + 1) per).  Empty
// normalised bins are never clipped, so with OpenCV's batch / residual / step (clahe.cpp; lut16_kernel) the cumulative
// LUT at normalised bin k is
//     C(k) + (k + 1) batch + min(residual, k / step + 1),   C(k) = sum over the occupied bins j <= k of min(h_j, clip)
// and only the occupied bins -- the values the frame has -- need it.
__global__ __launch_bounds__(256) void p16_table_kernel(const unsigned* mm, const unsigned* hist, int clip, float lut_scale,
                                                        uint16_t* lut) {
    __shared__ long long part[256];
    const int f = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    unsigned smin, smax;
    frame_range(mm, f, smin, smax);
    const int R = (int)(smax - smin) + 1;
    const NormMap16 nmap(smin, smax);
    const unsigned* hh = hist + (long long)f * kTableEntries + (long long)tile * R;
    uint16_t* tl = lut + (long long)f * kTableEntries + (long long)tile * R;
    const int per = (R + 255) / 256;
    auto head = [&](int i) {  // first raw bin >= i that starts a run of equal n
        if (i <= 0) return 0;
        if (i >= R) return R;
        unsigned prev = nmap(smin + i - 1);
        for (; i < R; ++i) {
            const unsigned k = nmap(smin + i);
            if (k != prev) break;
            prev = k;
        }
        return i;
    };
    const int b0 = head(t * per), b1 = head((t + 1) * per);
    // pass 1: what the thread's runs clip off, and their clipped sum
    long long over = 0, csum = 0;
    {
        long long run = 0;
        unsigned k = b0 < b1 ? nmap(smin + b0) : 0;
        for (int i = b0; i < b1; ++i) {
            run += hh[i];
            const unsigned kn = i + 1 < b1 ? nmap(smin + i + 1) : 0xffffffffu;
            if (kn != k) {
                if (clip > 0 && run > clip) {
                    over += run - clip;
                    run = clip;
                }
                csum += run;
                run = 0;
                k = kn;
            }
        }
    }
    part[t] = over;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    const long long clipped = part[0];
    __syncthreads();
    const long long batch = clip > 0 ? clipped / kBins16 : 0;
    const long long residual = clip > 0 ? clipped - batch * kBins16 : 0;
    const long long step = residual != 0 ? max(kBins16 / residual, 1LL) : 1;
    part[t] = csum;
    __syncthreads();
    if (t == 0) {
        long long acc = 0;
        for (int k = 0; k < 256; ++k) {
            const long long v = part[k];
            part[k] = acc;
            acc += v;
        }
    }
    __syncthreads();
    // pass 2: the cumulative LUT at each run's bin, stored for every raw value of the run
    long long c = part[t], run = 0;
    int start = b0;
    unsigned k = b0 < b1 ? nmap(smin + b0) : 0;
    for (int i = b0; i < b1; ++i) {
        run += hh[i];
        const unsigned kn = i + 1 < b1 ? nmap(smin + i + 1) : 0xffffffffu;
        if (kn != k) {
            c += clip > 0 && run > clip ? clip : run;
            const long long bonus = residual != 0 ? min(residual, (long long)k / step + 1) : 0;
            const long long sum = c + ((long long)k + 1) * batch + bonus;
            const uint16_t val = (uint16_t)sat_rint((float)sum * lut_scale, 65535.f);
            for (int j = start; j <= i; ++j) tl[j] = val;
            run = 0;
            start = i + 1;
            k = kn;
        }
    }
}

// the 8-bit value of pixel (x, y) (in the frame), the tile tables blended at that position or the raw value converted
struct Blend16 {
    Frames16 in;
    Geom16 g;
    float inv_tw, inv_th;  // 1.0f / tile size, rounded on the host (IEEE single division)
    const unsigned* mm;
    const uint16_t* lut;
};
template <bool CLAHE>
__device__ __forceinline__ unsigned pixel8(const Blend16& b, const uint16_t* img, const uint16_t* fl, unsigned smin, int R, int x,
                                           int y) {
    const unsigned v = img[(long long)y * b.in.stride + x];
    if (!CLAHE) return sat_rint(__fmul_rn((float)v, (float)(255. / 65535.)), 255.f);
    const float tyf = __fsub_rn(__fmul_rn((float)y, b.inv_th), 0.5f);
    int ty1 = (int)__builtin_floorf(tyf), ty2 = ty1 + 1;
    const float ya = __fsub_rn(tyf, (float)ty1), ya1 = __fsub_rn(1.0f, ya);
    ty1 = max(ty1, 0);
    ty2 = min(ty2, kTiles16 - 1);
    const float txf = __fsub_rn(__fmul_rn((float)x, b.inv_tw), 0.5f);
    int tx1 = (int)__builtin_floorf(txf), tx2 = tx1 + 1;
    const float xa = __fsub_rn(txf, (float)tx1), xa1 = __fsub_rn(1.0f, xa);
    tx1 = max(tx1, 0);
    tx2 = min(tx2, kTiles16 - 1);
    const unsigned i = v - smin;
    const float l11 = fl[(long long)(ty1 * kTiles16 + tx1) * R + i], l12 = fl[(long long)(ty1 * kTiles16 + tx2) * R + i];
    const float l21 = fl[(long long)(ty2 * kTiles16 + tx1) * R + i], l22 = fl[(long long)(ty2 * kTiles16 + tx2) * R + i];
    const float p11 = __fmul_rn(l11, xa1), p12 = __fmul_rn(l12, xa), p21 = __fmul_rn(l21, xa1), p22 = __fmul_rn(l22, xa);
    const float top = __fmul_rn(__fadd_rn(p11, p12), ya1), bot = __fmul_rn(__fadd_rn(p21, p22), ya);
    const unsigned r16 = sat_rint(__fadd_rn(top, bot), 65535.f);
    return sat_rint(__fmul_rn((float)r16, (float)(255. / 65535.)), 255.f);
}

// blend (or convert) only: grid (ceil(w / 256), ceil(h / 16), nframes), a thread = one column of 16 rows; dense output
template <bool CLAHE>
__global__ __launch_bounds__(256) void p16_blend_kernel(Blend16 b, uint8_t* out, unsigned long long* clk) {
    const bool probe = clk != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0;  // (mrgingham_amd_sclk_mhz)
    const ClockProbe clkp = clock_probe_begin(probe);
    const int f = blockIdx.z, x = blockIdx.x * 256 + threadIdx.x, y0 = blockIdx.y * 16, y1 = min(y0 + 16, b.in.h);
    const uint16_t* img = b.in.frames + (long long)f * b.in.pitch;
    const uint16_t* fl = b.lut + (long long)f * kTableEntries;
    unsigned smin = 0, smax = 0;
    if (CLAHE) frame_range(b.mm, f, smin, smax);
    const int R = (int)(smax - smin) + 1;
    uint8_t* o = out + (long long)f * b.in.w * b.in.h;
    if (x < b.in.w)
        for (int y = y0; y < y1; ++y) o[(long long)y * b.in.w + x] = (uint8_t)pixel8<CLAHE>(b, img, fl, smin, R, x, y);
    clock_probe_end(probe, clkp, clk);
}

// blend (or convert) + 3x3 box blur in one pass: grid (ceil(w / 256), ceil(h / 64), nframes).  The workgroup blends its
// 256 x 64 output pixels and the ring around them into LDS -- the ring is the BLENDED image's BORDER_REFLECT_101 (column
// -1 is column 1 blended at column 1), like cv::blur after clahe->apply -- then each thread rolls one column down the 64
// rows with the horizontal 3-sums of the last three rows.  The ring costs 4 % more blends than pixels.
constexpr int kBW = 256, kBH = 64, kPW = kBW + 2, kPH = kBH + 2;
template <bool CLAHE>
__global__ __launch_bounds__(256) void p16_blend_blur3_kernel(Blend16 b, uint8_t* out, unsigned long long* clk) {
    const bool probe = clk != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0;  // (mrgingham_amd_sclk_mhz)
    const ClockProbe clkp = clock_probe_begin(probe);
    __shared__ uint8_t patch[kPH * kPW];
    const int f = blockIdx.z, tid = threadIdx.x, W = b.in.w, H = b.in.h;
    const int bx0 = blockIdx.x * kBW, by0 = blockIdx.y * kBH;
    const uint16_t* img = b.in.frames + (long long)f * b.in.pitch;
    const uint16_t* fl = b.lut + (long long)f * kTableEntries;
    unsigned smin = 0, smax = 0;
    if (CLAHE) frame_range(b.mm, f, smin, smax);
    const int R = (int)(smax - smin) + 1;
    // samples: columns bx0 - 1 .. min(bx0 + 256, W), rows by0 - 1 .. min(by0 + 64, H) (the last ones only up to the frame's
    // reflected border row / column)
    const int pw = min(kBW, W - bx0) + 2, ph = min(kBH, H - by0) + 2;
    for (int j = tid; j < pw * ph; j += 256) {
        const int r = j / pw, c = j - r * pw;
        const int y = reflect101_16(by0 - 1 + r, H), x = reflect101_16(bx0 - 1 + c, W);
        patch[r * kPW + c] = (uint8_t)pixel8<CLAHE>(b, img, fl, smin, R, x, y);
    }
    __syncthreads();
    const int c = tid + 1;
    if (c < pw - 1) {
        uint8_t* o = out + (long long)f * W * H + (long long)by0 * W + bx0 + tid;
        auto hsum = [&](int r) { return (unsigned)patch[r * kPW + c - 1] + patch[r * kPW + c] + patch[r * kPW + c + 1]; };
        unsigned s0 = hsum(0), s1 = hsum(1);
        for (int r = 1; r < ph - 1; ++r) {
            const unsigned s2 = hsum(r + 1);
            o[(long long)(r - 1) * W] = (uint8_t)((s0 + s1 + s2 + 4) / 9);  // cv::blur 3x3: round to nearest (odd area, no ties)
            s0 = s1;
            s1 = s2;
        }
    }
    clock_probe_end(probe, clkp, clk);
}

}  // namespace

// scratch of one chunk of frames: extrema | tile histograms | composed LUTs, the tables laid out for R = 65 536
static size_t extrema_bytes(int nf) { return ((size_t)nf * 8 + 255) / 256 * 256; }
int preprocess16_batch_chunk_frames() {
    const int n = (int)(kPreprocess16TableBudget / ((size_t)kTableEntries * (4 + 2)));
    return n < 1 ? 1 : n;
}
size_t preprocess16_batch_scratch_bytes(int chunk_frames) {
    return extrema_bytes(chunk_frames) + (size_t)chunk_frames * kTableEntries * (4 + 2);
}

bool launch_preprocess16_batch(const uint16_t* frames, long long pitch, int nframes, int w, int h, int stride, bool do_clahe,
                               int blur_radius, uint8_t* out, void* scratch, uint8_t* tmp, hipStream_t s, unsigned long long* clk) {
    if (nframes <= 0 || w <= 0 || h <= 0) return true;
    Frames16 in{frames, pitch, w, h, stride, false};
    in.vec = w % 8 == 0 && stride % 8 == 0 && pitch % 8 == 0 && ((uintptr_t)frames & 15) == 0;
    const Geom16 g = geom16(w, h);
    if (do_clahe && (g.tw <= 0 || g.th <= 0)) return false;
    Blend16 bl{in, g, 1.0f / (float)(g.tw > 0 ? g.tw : 1), 1.0f / (float)(g.th > 0 ? g.th : 1), nullptr, nullptr};
    if (do_clahe) {
        const int chunk = preprocess16_batch_chunk_frames();
        const int nf = nframes < chunk ? nframes : chunk;  // (the caller's scratch holds this many frames' tables)
        unsigned* mm = (unsigned*)scratch;
        unsigned* hist = (unsigned*)((char*)scratch + extrema_bytes(nf));
        uint16_t* lut = (uint16_t*)(hist + (size_t)nf * kTableEntries);
        const long long area = (long long)g.tw * g.th;
        const float lut_scale = (float)(kBins16 - 1) / (float)area;
        const int clip = clip16(8.0, area);
        int rows = kSlabPixels / g.tw;  // rows of a histogram slab, balanced over the tile
        const int nslabs = (g.th + rows - 1) / rows;
        rows = (g.th + nslabs - 1) / nslabs;
        for (int f0 = 0; f0 < nframes; f0 += nf) {
            const int n = nframes - f0 < nf ? nframes - f0 : nf;
            Frames16 ci = in;
            ci.frames = frames + (long long)f0 * pitch;
            hipMemsetAsync(mm, 0xff, (size_t)n * 8, s);
            hipLaunchKernelGGL(p16_minmax_kernel, dim3((h + 15) / 16, n), dim3(256), 0, s, ci, mm);
            hipLaunchKernelGGL(p16_zero_kernel, dim3(kTileCount, n), dim3(256), 0, s, mm, hist);
            hipLaunchKernelGGL(p16_hist_small_kernel, dim3(nslabs, kTileCount, n), dim3(256), 0, s, ci, g, mm, hist, rows);
            hipLaunchKernelGGL(p16_hist_parts_kernel, dim3(kMaxParts, kTileCount, n), dim3(256), 0, s, ci, g, mm, hist);
            hipLaunchKernelGGL(p16_table_kernel, dim3(kTileCount, n), dim3(256), 0, s, mm, hist, clip, lut_scale, lut);
            Blend16 cb = bl;
            cb.in = ci;
            cb.mm = mm;
            cb.lut = lut;
            uint8_t* co = out + (long long)f0 * w * h;
            if (blur_radius == 1) {
                hipLaunchKernelGGL(p16_blend_blur3_kernel<true>, dim3((w + kBW - 1) / kBW, (h + kBH - 1) / kBH, n), dim3(256), 0, s,
                                   cb, co, clk);
            } else {
                uint8_t* bo = blur_radius > 0 ? tmp + (long long)f0 * w * h : co;
                hipLaunchKernelGGL(p16_blend_kernel<true>, dim3((w + 255) / 256, (h + 15) / 16, n), dim3(256), 0, s, cb, bo, clk);
                if (blur_radius > 0) launch_box_blur(FrameBatch{bo, (long long)w * h, w, h, w}, blur_radius, co, 0, n, s);
            }
        }
        return true;
    }
    if (blur_radius == 1) {
        hipLaunchKernelGGL(p16_blend_blur3_kernel<false>, dim3((w + kBW - 1) / kBW, (h + kBH - 1) / kBH, nframes), dim3(256), 0, s,
                           bl, out, clk);
    } else {
        uint8_t* bo = blur_radius > 0 ? tmp : out;
        hipLaunchKernelGGL(p16_blend_kernel<false>, dim3((w + 255) / 256, (h + 15) / 16, nframes), dim3(256), 0, s, bl, bo, clk);
        if (blur_radius > 0) launch_box_blur(FrameBatch{bo, (long long)w * h, w, h, w}, blur_radius, out, 0, nframes, s);
    }
    return true;
}

}  // namespace mrg
