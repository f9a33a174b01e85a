// ref_harness.cc -- TEST INFRASTRUCTURE ONLY.
//
// extern "C" entry points over the three upstream symbols of find_chessboard_corners.hh, which oracle/Makefile
// (target `ref`) finds in the reference tree by -I and compiles, unmodified and where it lies, against the
// stand-in headers of oracle/ref_stub.  Nothing upstream is copied here.  Two libraries come out:
//
//   _ref/libfcc_ref.so       this file + the upstream .cc + the upstream ChESS.c (compiled as C):
//                            fcc_ref_detect / fcc_ref_refine run the upstream path on an IMAGE;
//   _ref/libfcc_resp_ref.so  this file with -DFCC_REF_ON_RESPONSE + the upstream .cc: the
//                            mrgingham_ChESS_response_5 that the upstream file calls is the one below, which copies
//                            a response set by the caller, so fcc_ref_cc_*_on_response run the upstream component
//                            search on a HAND-BUILT response.
//
// Above level 0 the upstream file calls cv::resize; the stand-in's resize computes nothing and asks
// fcc_ref_resize_hook for the level image that the caller passed in.  `debug` is always false: with it set the
// upstream file writes under /tmp.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "find_chessboard_corners.hh"

namespace {
const unsigned char* g_level_image = NULL;
int g_level_rows = 0, g_level_cols = 0;

void set_level_image(const uint8_t* p, int rows, int cols)
{
    g_level_image = p;
    g_level_rows = rows;
    g_level_cols = cols;
}

int detect(int32_t* xy_out, int cap, const cv::Mat& image, int level)
{
    std::vector<mrgingham::PointInt> points;
    const int zeros_before = fcc_ref_zeros_calls;
    mrgingham::find_chessboard_corners_from_image_array(&points, image, level, false, NULL);
    if (fcc_ref_zeros_calls == zeros_before) return -1;   // upstream gave up before it had a level image
    const int n = (int)points.size();
    for (int i = 0; i < n && i < cap; i++) {
        xy_out[2 * i + 0] = points[i].x;
        xy_out[2 * i + 1] = points[i].y;
    }
    return n;
}

int refine(double* xy, signed char* levels, int npoints, const cv::Mat& image, int level)
{
    std::vector<mrgingham::PointDouble> points((size_t)npoints);
    for (int i = 0; i < npoints; i++) points[i] = mrgingham::PointDouble(xy[2 * i + 0], xy[2 * i + 1]);
    const int nrefined = mrgingham::refine_chessboard_corners_from_image_array(&points, levels, image, level, false, NULL);
    for (int i = 0; i < npoints; i++) {
        xy[2 * i + 0] = points[i].x;
        xy[2 * i + 1] = points[i].y;
    }
    return nrefined;
}
}  // namespace

extern "C" {

int fcc_ref_zeros_calls = 0;

const unsigned char* fcc_ref_resize_hook(int* rows, int* cols)
{
    *rows = g_level_rows;
    *cols = g_level_cols;
    return g_level_image;
}

#ifndef FCC_REF_ON_RESPONSE

// Points x1000 in upstream order.  Returns their number (which may exceed `cap`; then only `cap` were written), or -1
// where upstream returned before it had a level image (level out of range, non-continuous level-0 input).
// `level_image` (lh x lw, dense) is what cv::resize hands back; unused at level 0.
__attribute__((visibility("default")))
int fcc_ref_detect(int32_t* xy_out, int cap, const uint8_t* image, int H, int W, int stride, int level,
                   const uint8_t* level_image, int lh, int lw)
{
    set_level_image(level_image, lh, lw);
    const cv::Mat m(H, W, CV_8U, (void*)image, (size_t)stride);
    return detect(xy_out, cap, m, level);
}

// xy and levels are updated in place; returns upstream's count of refined points.
__attribute__((visibility("default")))
int fcc_ref_refine(double* xy, signed char* levels, int npoints, const uint8_t* image, int H, int W, int stride,
                   int level, const uint8_t* level_image, int lh, int lw)
{
    set_level_image(level_image, lh, lw);
    const cv::Mat m(H, W, CV_8U, (void*)image, (size_t)stride);
    return refine(xy, levels, npoints, m, level);
}

#else  // FCC_REF_ON_RESPONSE

static const int16_t* g_response = NULL;

// The signature of ChESS.h.  Upstream calls this with its zeroed w x h buffer; it receives the caller's response.
void mrgingham_ChESS_response_5(int16_t* response, const uint8_t* image, int w, int h, int stride)
{
    (void)image;
    (void)stride;
    memcpy(response, g_response, sizeof(int16_t) * (size_t)w * (size_t)h);
}

// The upstream file takes the level image as it is at level 0 and from cv::resize above it; either way it is
// `level_image`, w x h, and `d` is the response it then searches.  The input Mat's own size is read nowhere else.
static cv::Mat response_call(const int16_t* d, const uint8_t* level_image, int w, int h)
{
    g_response = d;
    set_level_image(level_image, h, w);
    return cv::Mat(h, w, CV_8U, (void*)level_image, (size_t)w);
}

// Arguments of oracle_cc_detect_on_response; `d` is not modified (upstream searches its own copy).
__attribute__((visibility("default")))
int fcc_ref_cc_detect_on_response(int32_t* xy_out, int cap, const int16_t* d, const uint8_t* level_image, int w, int h,
                                  int level)
{
    const cv::Mat m = response_call(d, level_image, w, h);
    return detect(xy_out, cap, m, level);
}

// Arguments of oracle_cc_refine_on_response.
__attribute__((visibility("default")))
int fcc_ref_cc_refine_on_response(double* xy, signed char* levels, int npoints, const int16_t* d,
                                  const uint8_t* level_image, int w, int h, int level)
{
    const cv::Mat m = response_call(d, level_image, w, h);
    return refine(xy, levels, npoints, m, level);
}

#endif

}  // extern "C"
