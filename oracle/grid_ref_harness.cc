// grid_ref_harness.cc -- TEST INFRASTRUCTURE ONLY.
//
// extern "C" entry points over the upstream mrgingham::find_grid_from_points, which oracle/Makefile (target `ref`)
// finds in the reference tree and compiles, unmodified and where it lies, against the stand-in
// oracle/ref_stub/boost/polygon/voronoi.hpp (and the stand-in opencv2/ that mrgingham.hh pulls in).  Nothing
// upstream is copied here.  Out comes _ref/libgrid_ref.so.
//
// `debug` is always false: with it set the upstream file writes under /tmp.
#include <stdint.h>

#include <vector>

#include <boost/polygon/voronoi.hpp>

#include "point.hh"
#include "mrgingham.hh"

extern "C" {
// where every cell's incident_edge() starts (see the stand-in): 0 = canonical, else a hashed rotation
unsigned grid_ref_ring_start = 0;
}

// a point type of this file's own for grid_ref_rings (the upstream file specialises the traits of PointInt itself)
namespace { struct RingPoint { int x, y; }; }
namespace boost { namespace polygon {
template <> struct geometry_concept<RingPoint> { typedef point_concept type; };
template <> struct point_traits<RingPoint> {
    typedef int coordinate_type;
    static inline coordinate_type get(const RingPoint& p, orientation_2d o) { return o == HORIZONTAL ? p.x : p.y; }
};
}}

namespace {
bool in_range(const int32_t* xy, int n)
{
    for (int i = 0; i < 2 * n; i++)
        if (xy[i] <= -(1 << 28) || xy[i] >= (1 << 28)) return false;   // the stand-in's exact predicates
    return true;
}
}  // namespace

extern "C" {

// xy: n points x1000; out: gridn * gridn points.  1 = board found, 0 = none, -1 = bad arguments.
__attribute__((visibility("default")))
int grid_ref_find(double* xy_out, const int32_t* xy, int n, int gridn, unsigned ring_start)
{
    if (n < 0 || gridn < 2 || !in_range(xy, n)) return -1;
    std::vector<mrgingham::PointInt> pts((size_t)n);
    for (int i = 0; i < n; i++) pts[i] = mrgingham::PointInt(xy[2 * i], xy[2 * i + 1]);
    std::vector<mrgingham::PointDouble> out;
    grid_ref_ring_start = ring_start;
    const bool ok = mrgingham::find_grid_from_points(out, pts, gridn, false);
    grid_ref_ring_start = 0;
    if (!ok) return 0;
    if ((int)out.size() != gridn * gridn) return -1;
    for (int i = 0; i < gridn * gridn; i++) {
        xy_out[2 * i] = out[i].x;
        xy_out[2 * i + 1] = out[i].y;
    }
    return 1;
}

// The stand-in's diagram by itself.  Cells in order: cell_source[c] = source_index(), cell_first[c] = index of its
// incident edge (-1: none); edges in ring order from the incident edge, cell after cell: edge_cell / edge_nbr (the
// cell of the twin) / edge_twin / edge_next / edge_prev as indices (-1: a null pointer).  Returns the number of
// edges (written up to edge_cap), *ncells the number of cells (written up to cell_cap); -1 = bad arguments.
__attribute__((visibility("default")))
int grid_ref_rings(const int32_t* xy, int n, unsigned ring_start, int* ncells, int* cell_source, int* cell_first,
                   int cell_cap, int* edge_cell, int* edge_nbr, int* edge_twin, int* edge_next, int* edge_prev,
                   int edge_cap)
{
    if (n < 0 || !in_range(xy, n)) return -1;
    std::vector<RingPoint> pts((size_t)n);
    for (int i = 0; i < n; i++) { pts[i].x = xy[2 * i]; pts[i].y = xy[2 * i + 1]; }
    typedef boost::polygon::voronoi_diagram<double> VD;
    VD vd;
    grid_ref_ring_start = ring_start;
    boost::polygon::construct_voronoi(pts.begin(), pts.end(), &vd);
    grid_ref_ring_start = 0;
    const VD::cell_type* c0 = vd.cells().empty() ? NULL : &vd.cells()[0];
    // ring-order numbering of the edges
    std::vector<const VD::edge_type*> order;
    std::vector<int> first(vd.cells().size(), -1);
    for (size_t c = 0; c < vd.cells().size(); c++) {
        const VD::edge_type* e0 = vd.cells()[c].incident_edge();
        if (!e0) continue;
        first[c] = (int)order.size();
        const VD::edge_type* e = e0;
        do {
            order.push_back(e);
            e = e->next();
        } while (e && e != e0 && order.size() < vd.edges_.size() + 1);
    }
    std::vector<int> number(vd.edges_.size(), -1);
    for (size_t k = 0; k < order.size(); k++) {
        const size_t at = (size_t)(order[k] - &vd.edges_[0]);
        if (at < number.size() && number[at] < 0) number[at] = (int)k;
    }
    auto idx = [&](const VD::edge_type* e) { return e ? number[(size_t)(e - &vd.edges_[0])] : -1; };
    *ncells = (int)vd.cells().size();
    for (size_t c = 0; c < vd.cells().size() && (int)c < cell_cap; c++) {
        cell_source[c] = (int)vd.cells()[c].source_index();
        cell_first[c] = first[c];
    }
    for (size_t k = 0; k < order.size() && (int)k < edge_cap; k++) {
        const VD::edge_type* e = order[k];
        edge_cell[k] = e->cell() ? (int)(e->cell() - c0) : -1;
        edge_nbr[k] = e->twin() && e->twin()->cell() ? (int)(e->twin()->cell() - c0) : -1;
        edge_twin[k] = idx(e->twin());
        edge_next[k] = idx(e->next());
        edge_prev[k] = idx(e->prev());
    }
    return (int)order.size();
}

}  // extern "C"
