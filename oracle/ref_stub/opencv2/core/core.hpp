// REFERENCE-BUILD STAND-IN, not OpenCV -- TEST INFRASTRUCTURE ONLY.
//
// The structural part of cv:: that the upstream find_chessboard_corners.cc and find_chessboard_corners.hh
// touch, so that the upstream file compiles UNMODIFIED where it lies (oracle/Makefile, target `ref`) in an
// image without OpenCV.  No OpenCV arithmetic is restated here:
//   * at pyramid level 0 the upstream file reads only Mat fields and Mat::zeros;
//   * above level 0 its one OpenCV call is cv::resize, and this resize computes NOTHING: it asks the
//     harness (oracle/ref_harness.cc) for the level image that the caller of the harness passed in and
//     installs it.  What the reference build pins is therefore the component search and the coordinate
//     scaling at every level, and the whole path only at level 0 -- never the resize formula;
//   * normalize / imwrite / imread exist for the debug and file paths, which the harness never takes.
//
// How this differs from tests/boundary/opencv2/core/core.hpp: that one holds the four Mat members the
// project's own shim header touches and exists so the shim can be compiled; nothing runs through it.
// This one is run: the upstream component search executes over these Mats.
#pragma once
// the real headers bring these in transitively and the upstream file relies on it
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_16S 3

extern "C" {
// Defined by oracle/ref_harness.cc.
// The level image of the call in flight: its pixels (dense rows) and its size.
const unsigned char* fcc_ref_resize_hook(int* rows, int* cols);
// Counts Mat::zeros calls: upstream allocates its response only after the level image was accepted
// (find_chessboard_corners.cc:495-506), so the harness can tell upstream's error return from "no corners".
extern int fcc_ref_zeros_calls;
}

namespace cv {

enum { INTER_LINEAR = 1 };
enum { NORM_MINMAX = 32 };
enum { IMREAD_GRAYSCALE = 0, IMREAD_IGNORE_ORIENTATION = 128 };

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

struct Mat {
    int rows, cols;
    unsigned char* data;
    size_t step;

    Mat() : rows(0), cols(0), data(NULL), step(0), type_(CV_8U) {}
    // a view of the caller's pixels; nothing is copied or owned
    Mat(int r, int c, int t, void* d, size_t s) : rows(r), cols(c), data((unsigned char*)d), step(s), type_(t) {}

    static Mat zeros(Size size, int type)
    {
        fcc_ref_zeros_calls++;
        const size_t elem = (type == CV_16S) ? 2 : 1;
        const size_t bytes = (size_t)size.width * (size_t)size.height * elem;
        Mat m;
        m.owner_.reset((unsigned char*)calloc(bytes ? bytes : 1, 1), free);
        m.rows = size.height;
        m.cols = size.width;
        m.data = m.owner_.get();
        m.step = (size_t)size.width * elem;
        m.type_ = type;
        return m;
    }

    int type() const { return type_; }
    bool isContinuous() const { return rows <= 1 || step == (size_t)cols * (type_ == CV_16S ? 2 : 1); }

private:
    int type_;
    std::shared_ptr<unsigned char> owner_;
};

// No arithmetic: dst becomes a view of the level image the harness holds for this call.
inline void resize(const Mat&, Mat& dst, Size, double, double, int)
{
    int rows = 0, cols = 0;
    const unsigned char* p = fcc_ref_resize_hook(&rows, &cols);
    dst = Mat(rows, cols, CV_8U, (void*)p, (size_t)cols);
}

inline void normalize(const Mat&, Mat&, double, double, int) {}
inline bool imwrite(const std::string&, const Mat&) { return false; }
inline Mat imread(const std::string&, int) { return Mat(); }

}  // namespace cv
