// Stand-in for <boost/polygon/voronoi.hpp> -- TEST INFRASTRUCTURE ONLY.
//
// Written from boost.polygon's documented interface, for one client: the upstream find_grid.cc, which oracle/Makefile
// (target `ref`) compiles where it lies.  It provides the names that file uses and nothing else of boost:
//   geometry_concept / point_concept / point_traits / orientation_2d / HORIZONTAL   (the client specialises them)
//   voronoi_diagram<double> with cell_type, edge_type and cells()
//   cell_type::source_index(), incident_edge();  edge_type::cell(), twin(), next(), prev()
//   construct_voronoi(first, last, &vd)
//
// construct_voronoi builds the half-edge structure of the Voronoi diagram of integer point sites:
//   - cells in the order of the sites sorted by (x, then y); coincident points share one cell (its source_index
//     is the smallest input index among them);
//   - two sites share an edge exactly when their Voronoi edge has positive length: the Delaunay edges, an exactly
//     cocircular quadruple gets NO diagonal, collinear sites are joined only to their direct neighbours on the line;
//   - next() goes counter-clockwise round the cell's site, in (x, y) taken as numbers; prev() the other way;
//   - the ring of a hull cell is closed (boost links the two infinite edges to each other);
//   - every predicate is exact (__int128; coordinates must stay below 2^28 in magnitude).
// The construction wraps each cell by itself: the nearest site is a neighbour; from a neighbour j of site i the
// next one counter-clockwise is the site left of i->j whose circle through i and j holds no other such site (of
// several on one circle, the last one counter-clockwise as seen from i); a site whose left side is empty continues
// with the nearest site exactly opposite, or is on the hull.  O(n * degree) per site, no sweep, no flips: it shares
// no method with the product's triangulation (mrgingham_amd/csrc/grid.cpp) and is a second witness, not a copy.
//
// Where a cell's ring STARTS (incident_edge()) is an implementation detail of boost.  Here the harness chooses it
// through grid_ref_ring_start: 0 = the canonical start, the first neighbour counter-clockwise from the +x direction
// (+x itself included); any other value rotates the ring from there by a hash of the value and the cell's source index,
// the hash of the product's GridPerturbation::ring_seed.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <iterator>
#include <vector>

extern "C" unsigned grid_ref_ring_start;

namespace boost { namespace polygon {

struct point_concept {};
template <typename T> struct geometry_concept {};
enum orientation_2d { HORIZONTAL = 0, VERTICAL = 1 };
template <typename T> struct point_traits {};

template <typename T> class voronoi_edge;

template <typename T>
class voronoi_cell {
public:
    typedef voronoi_edge<T> voronoi_edge_type;
    voronoi_cell() : source_index_(0), incident_edge_(NULL) {}
    size_t source_index() const { return source_index_; }
    const voronoi_edge_type* incident_edge() const { return incident_edge_; }

    size_t source_index_;
    voronoi_edge_type* incident_edge_;
};

template <typename T>
class voronoi_edge {
public:
    typedef voronoi_cell<T> voronoi_cell_type;
    voronoi_edge() : cell_(NULL), twin_(NULL), next_(NULL), prev_(NULL) {}
    const voronoi_cell_type* cell() const { return cell_; }
    const voronoi_edge* twin() const { return twin_; }
    const voronoi_edge* next() const { return next_; }
    const voronoi_edge* prev() const { return prev_; }

    voronoi_cell_type* cell_;
    voronoi_edge *twin_, *next_, *prev_;
};

template <typename T>
class voronoi_diagram {
public:
    typedef voronoi_cell<T> cell_type;
    typedef voronoi_edge<T> edge_type;
    typedef std::vector<cell_type> cell_container_type;
    const cell_container_type& cells() const { return cells_; }

    cell_container_type cells_;
    std::vector<edge_type> edges_;
};

namespace stand_in {

typedef long long i64;
typedef __int128 i128;
struct Site { i64 x, y; size_t source; };

// > 0: c left of a -> b
inline int orient(const Site& a, const Site& b, const Site& c)
{
    const i128 d = (i128)(b.x - a.x) * (c.y - a.y) - (i128)(b.y - a.y) * (c.x - a.x);
    return d > 0 ? 1 : (d < 0 ? -1 : 0);
}

// a, b, c counter-clockwise; > 0: d strictly inside their circle, 0: on it
inline int incircle(const Site& a, const Site& b, const Site& c, const Site& d)
{
    const i128 ax = a.x - d.x, ay = a.y - d.y, bx = b.x - d.x, by = b.y - d.y, cx = c.x - d.x, cy = c.y - d.y;
    const i128 det = (ax * ax + ay * ay) * (bx * cy - by * cx) - (bx * bx + by * by) * (ax * cy - ay * cx) +
                     (cx * cx + cy * cy) * (ax * by - ay * bx);
    return det > 0 ? 1 : (det < 0 ? -1 : 0);
}

inline i128 dist2(const Site& a, const Site& b)
{
    return (i128)(a.x - b.x) * (a.x - b.x) + (i128)(a.y - b.y) * (a.y - b.y);
}

// The neighbour of site i that follows its neighbour j, counter-clockwise (ccw = true) or clockwise; -1: none (hull).
inline int next_round(const std::vector<Site>& s, int i, int j, bool ccw)
{
    const int side = ccw ? 1 : -1;
    int best = -1;
    for (int k = 0; k < (int)s.size(); ++k) {
        if (k == i || k == j || orient(s[i], s[j], s[k]) != side) continue;
        if (best < 0) { best = k; continue; }
        const int in = ccw ? incircle(s[i], s[j], s[best], s[k]) : incircle(s[j], s[i], s[best], s[k]);
        if (in > 0 || (in == 0 && orient(s[i], s[best], s[k]) == side)) best = k;
    }
    if (best >= 0) return best;
    // nothing on that side: the nearest site exactly opposite j is the next one (half a turn on)
    for (int k = 0; k < (int)s.size(); ++k) {
        if (k == i || k == j || orient(s[i], s[j], s[k]) != 0) continue;
        if ((i128)(s[j].x - s[i].x) * (s[k].x - s[i].x) + (i128)(s[j].y - s[i].y) * (s[k].y - s[i].y) > 0) continue;
        if (best < 0 || dist2(s[i], s[k]) < dist2(s[i], s[best])) best = k;
    }
    return best;
}

// the neighbours of site i, counter-clockwise
inline void ring_of(const std::vector<Site>& s, int i, std::vector<int>& ring)
{
    ring.clear();
    const int n = (int)s.size();
    int j0 = -1;
    for (int k = 0; k < n; ++k)
        if (k != i && (j0 < 0 || dist2(s[i], s[k]) < dist2(s[i], s[j0]))) j0 = k;
    if (j0 < 0) return;
    ring.push_back(j0);
    bool closed = false;
    for (int j = j0; (int)ring.size() <= n;) {
        j = next_round(s, i, j, true);
        if (j == j0) { closed = true; break; }
        if (j < 0) break;
        ring.push_back(j);
    }
    if (closed) return;
    std::vector<int> back;
    for (int j = j0; (int)back.size() <= n;) {
        j = next_round(s, i, j, false);
        if (j < 0) break;
        back.push_back(j);
    }
    ring.insert(ring.begin(), back.rbegin(), back.rend());
}

// 0: direction in [0, pi) from +x, 1: in [pi, 2 pi)
inline int half(i64 dx, i64 dy) { return (dy > 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

}  // namespace stand_in

template <typename PointIterator, typename VD>
void construct_voronoi(PointIterator first, PointIterator last, VD* vd)
{
    using namespace stand_in;
    typedef typename std::iterator_traits<PointIterator>::value_type Point;
    std::vector<Site> all;
    size_t idx = 0;
    for (PointIterator it = first; it != last; ++it, ++idx) {
        Site st;
        st.x = point_traits<Point>::get(*it, HORIZONTAL);
        st.y = point_traits<Point>::get(*it, VERTICAL);
        st.source = idx;
        all.push_back(st);
    }
    std::sort(all.begin(), all.end(), [](const Site& a, const Site& b) {
        return a.x != b.x ? a.x < b.x : (a.y != b.y ? a.y < b.y : a.source < b.source);
    });
    std::vector<Site> s;
    for (size_t k = 0; k < all.size(); ++k)
        if (s.empty() || s.back().x != all[k].x || s.back().y != all[k].y) s.push_back(all[k]);
    const int n = (int)s.size();

    std::vector<std::vector<int> > rings((size_t)n);
    std::vector<size_t> off((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        ring_of(s, i, rings[i]);
        off[i + 1] = off[i] + rings[i].size();
    }
    vd->cells_.assign((size_t)n, typename VD::cell_type());
    vd->edges_.assign(off[n], typename VD::edge_type());
    for (int i = 0; i < n; ++i) {
        typename VD::cell_type& c = vd->cells_[i];
        c.source_index_ = s[i].source;
        const std::vector<int>& r = rings[i];
        const int deg = (int)r.size();
        if (!deg) continue;
        for (int k = 0; k < deg; ++k) {
            typename VD::edge_type& e = vd->edges_[off[i] + k];
            e.cell_ = &c;
            e.next_ = &vd->edges_[off[i] + (k + 1) % deg];
            e.prev_ = &vd->edges_[off[i] + (k + deg - 1) % deg];
            const std::vector<int>& rj = rings[r[k]];
            for (size_t q = 0; q < rj.size(); ++q)
                if (rj[q] == i) e.twin_ = &vd->edges_[off[r[k]] + q];
        }
        // the canonical start: the smallest direction angle in [0, 2 pi)
        int start = 0;
        for (int k = 1; k < deg; ++k) {
            const i64 ax = s[r[k]].x - s[i].x, ay = s[r[k]].y - s[i].y;
            const i64 bx = s[r[start]].x - s[i].x, by = s[r[start]].y - s[i].y;
            const int ha = half(ax, ay), hb = half(bx, by);
            if (ha != hb ? ha < hb : (i128)ax * by - (i128)ay * bx > 0) start = k;
        }
        if (grid_ref_ring_start) {
            uint32_t hsh = (uint32_t)s[i].source * 2654435761u ^ (uint32_t)grid_ref_ring_start;
            hsh ^= hsh >> 15; hsh *= 0x2c1b3c6du; hsh ^= hsh >> 12;
            start = (start + (int)(hsh % (uint32_t)deg)) % deg;
        }
        c.incident_edge_ = &vd->edges_[off[i] + start];
    }
}

}}  // namespace boost::polygon
