// tgs_mesh_sdf.hpp -- signed distance from points to a triangle mesh: the per-pair functions, the bounding-volume tree and its host build, and the
// per-point walks, shared by the device kernels (tgs_mesh_sdf.hip), the host twin (tgs_meshsdf_query_host) and the stand-alone host check
// (tools/mesh_sdf_host_check.cpp).  Plain C++17: no HIP header, no other header of this library, so a host compiler takes it as it is.
// include/tgs_raster.h ("mesh signed distance") has the rules in full; tests/mesh_sdf_ref.py restates them in numpy float64.
//
// All arithmetic is in double on the float32 inputs and is compiled without contraction (the pragma below, and -ffp-contract=off on the file), so
// the host build and the device build evaluate the same expressions: no fma where the source has a multiply and an add.
#ifndef TGS_MESH_SDF_HPP
#define TGS_MESH_SDF_HPP

#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define TGS_SDF_HD __host__ __device__ inline
#else
#define TGS_SDF_HD inline
#endif

namespace tgs {
namespace msdf {

constexpr uint32_t MAGIC = 0x46445354u;        // "TSDF"
constexpr int LEAF_FACES = 4;                  // faces per leaf, at most
constexpr int MAX_DEPTH = 32;                  // median splits halve: F < 2^28 faces reach a leaf within 27 levels; the build checks it
constexpr int MAX_FACES = (1 << 28) - 1;       // a leaf's word holds 8 * first + count in 31 bits
constexpr size_t HEADER_BYTES = 64;

struct Header {                                // 64 bytes at the start of the tree
    uint32_t magic, n_faces, n_nodes, depth;
    uint32_t leaf_faces, reserved[11];
};
struct Node {                                  // 32 bytes.  Depth-first order: the left child of an inner node i is i + 1, the right child is nodes[i + 1].skip
    float lo[3], hi[3];                        // the box, rounded outward
    int32_t skip;                              // the node that follows this node's subtree (a leaf: i + 1)
    int32_t leaf;                              // -1: an inner node; else 8 * (the first record) + (the number of records, 1..LEAF_FACES)
};
struct Record {                                // 64 bytes: one face as a leaf holds it, in leaf order
    float v[9];                                // the three vertices
    int32_t idx[3];                            // their indices (the canonical direction of an edge is from the lower one)
    int32_t face;                              // the face's number in the caller's array
    int32_t pad[3];
};
static_assert(sizeof(Header) == 64 && sizeof(Node) == 32 && sizeof(Record) == 64, "tree layout");

TGS_SDF_HD size_t tree_bytes(size_t F) { return HEADER_BYTES + sizeof(Node) * 2 * F + sizeof(Record) * F; }
TGS_SDF_HD const Node* tree_nodes(const void* tree) { return (const Node*)((const char*)tree + HEADER_BYTES); }
TGS_SDF_HD const Record* tree_records(const void* tree, size_t F) { return (const Record*)((const char*)tree + HEADER_BYTES + sizeof(Node) * 2 * F); }

struct D3 { double x, y, z; };
TGS_SDF_HD D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
TGS_SDF_HD double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
TGS_SDF_HD D3 axpy(D3 a, double t, D3 d) { return {a.x + t * d.x, a.y + t * d.y, a.z + t * d.z}; }
TGS_SDF_HD D3 load3(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
TGS_SDF_HD bool finite1(float x) { return x - x == 0.0f; }                      // false for NaN and for either infinity
TGS_SDF_HD bool finite3(const float* p) { return finite1(p[0]) && finite1(p[1]) && finite1(p[2]); }

// ---- pair function 1: the closest point of a triangle ---------------------------------------------------------------------------------
TGS_SDF_HD D3 closest_on_segment(D3 p, D3 a, D3 b)
{
    const D3 ab = sub(b, a);
    const double den = dot(ab, ab);
    double t = den > 0.0 ? dot(sub(p, a), ab) / den : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    return axpy(a, t, ab);
}
TGS_SDF_HD double dist2(D3 p, D3 c) { const D3 d = sub(p, c); return dot(d, d); }

// the three segments ab, bc, ca in this order, the first of the nearest: a face whose cross product is exactly zero, and the way out for a
// sliver whose barycentric denominator is not positive
TGS_SDF_HD D3 closest_on_segments(D3 p, D3 a, D3 b, D3 c)
{
    D3 best = closest_on_segment(p, a, b);
    double bd = dist2(p, best);
    const D3 c1 = closest_on_segment(p, b, c);
    const double d1 = dist2(p, c1);
    if (d1 < bd) { bd = d1; best = c1; }
    const D3 c2 = closest_on_segment(p, c, a);
    if (dist2(p, c2) < bd) best = c2;
    return best;
}

// the closest point of triangle (a, b, c) to p: the vertex, edge and face regions by the signs of the six projections (Ericson, Real-Time
// Collision Detection, 5.1.5)
TGS_SDF_HD D3 closest_on_triangle(D3 p, D3 a, D3 b, D3 c)
{
    const D3 ab = sub(b, a), ac = sub(c, a);
    const double nx = ab.y * ac.z - ab.z * ac.y, ny = ab.z * ac.x - ab.x * ac.z, nz = ab.x * ac.y - ab.y * ac.x;
    if (nx == 0.0 && ny == 0.0 && nz == 0.0) return closest_on_segments(p, a, b, c);
    const D3 ap = sub(p, a);
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return a;
    const D3 bp = sub(p, b);
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return b;
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) return axpy(a, d1 / (d1 - d3), ab);
    const D3 cp = sub(p, c);
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return c;
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) return axpy(a, d2 / (d2 - d6), ac);
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) return axpy(b, (d4 - d3) / ((d4 - d3) + (d5 - d6)), sub(c, b));
    const double s = (va + vb) + vc;
    if (!(s > 0.0)) return closest_on_segments(p, a, b, c);
    const double v = vb / s, w = vc / s;
    return {(a.x + ab.x * v) + ac.x * w, (a.y + ab.y * v) + ac.y * w, (a.z + ab.z * v) + ac.z * w};
}

// ---- pair function 2: does the ray from p along +k cross the face? ---------------------------------------------------------------------
// (a, b) are the other two axes in cyclic order.  One edge from vertex (ia; xa, ya) to vertex (ib; xb, yb) in the face's order, the point
// (pa, pb): the edge value on the edge's canonical direction (from the lower index), its sign flipped for the face that runs it the other
// way; an exact zero takes the sign of -(V_b - U_b), then of (V_a - U_a).  -> the oriented value in e, the oriented sign (0: no side).
TGS_SDF_HD int edge_side(int ia, double xa, double ya, int ib, double xb, double yb, double pa, double pb, double& e)
{
    if (ia == ib) { e = 0.0; return 0; }
    const bool fwd = ia < ib;
    const double ua = fwd ? xa : xb, ub = fwd ? ya : yb, va = fwd ? xb : xa, vb = fwd ? yb : ya;
    const double E = (va - ua) * (pb - ub) - (vb - ub) * (pa - ua);
    int s = E > 0.0 ? 1 : (E < 0.0 ? -1 : 0);
    if (s == 0) {
        const double t = -(vb - ub);
        s = t > 0.0 ? 1 : (t < 0.0 ? -1 : 0);
        if (s == 0) { const double u = va - ua; s = u > 0.0 ? 1 : (u < 0.0 ? -1 : 0); }
    }
    e = fwd ? E : -E;
    return fwd ? s : -s;
}

template <int K> TGS_SDF_HD double comp(D3 v) { return K == 0 ? v.x : (K == 1 ? v.y : v.z); }

// 1: the face's projection onto (a, b) contains the point (three oriented signs equal and not zero), the three values do not sum to zero, and
// the face's height over the point -- the k coordinates combined with the edge values as weights -- is > p_k
template <int K>
TGS_SDF_HD int crossing(D3 p, D3 v0, D3 v1, D3 v2, int i0, int i1, int i2)
{
    constexpr int A = (K + 1) % 3, B = (K + 2) % 3;
    const double pa = comp<A>(p), pb = comp<B>(p);
    double e0, e1, e2;
    const int s0 = edge_side(i0, comp<A>(v0), comp<B>(v0), i1, comp<A>(v1), comp<B>(v1), pa, pb, e0);
    const int s1 = edge_side(i1, comp<A>(v1), comp<B>(v1), i2, comp<A>(v2), comp<B>(v2), pa, pb, e1);
    const int s2 = edge_side(i2, comp<A>(v2), comp<B>(v2), i0, comp<A>(v0), comp<B>(v0), pa, pb, e2);
    if (s0 == 0 || s0 != s1 || s0 != s2) return 0;
    const double sum = (e0 + e1) + e2;
    if (sum == 0.0) return 0;
    const double h = ((e0 * comp<K>(v2) + e1 * comp<K>(v0)) + e2 * comp<K>(v1)) / sum;
    return h > comp<K>(p) ? 1 : 0;
}

// ---- pair function 3: a lower bound of the squared distance from p to a box ------------------------------------------------------------
TGS_SDF_HD double gap(double p, double lo, double hi) { return p < lo ? lo - p : (p > hi ? p - hi : 0.0); }
TGS_SDF_HD double box_lower_bound(D3 p, const Node& n)
{
    const double gx = gap(p.x, (double)n.lo[0], (double)n.hi[0]), gy = gap(p.y, (double)n.lo[1], (double)n.hi[1]), gz = gap(p.z, (double)n.lo[2], (double)n.hi[2]);
    // the boxes are padded by 2^-20 of the mesh's largest coordinate, which covers the rounding of a computed distance near the mesh; far from
    // it that rounding is relative, and so is this factor: the bound stays below every computed distance of a face in the box
    return ((gx * gx + gy * gy) + gz * gz) * (1.0 - 0x1p-30);
}
// may the ray from p along some axis cross a face in the box?  bit k: the box's (a, b) extent contains the point and its upper k bound is > p_k
TGS_SDF_HD int box_ray_axes(D3 p, const Node& n)
{
    const bool ix = p.x >= (double)n.lo[0] && p.x <= (double)n.hi[0], iy = p.y >= (double)n.lo[1] && p.y <= (double)n.hi[1], iz = p.z >= (double)n.lo[2] && p.z <= (double)n.hi[2];
    return ((iy && iz && (double)n.hi[0] > p.x) ? 1 : 0) | ((iz && ix && (double)n.hi[1] > p.y) ? 2 : 0) | ((ix && iy && (double)n.hi[2] > p.z) ? 4 : 0);
}

// ---- one point's state and the update every walk makes ---------------------------------------------------------------------------------
struct Best {
    double d2;                                 // the least squared distance so far
    D3 c;                                      // that face's closest point
    int face;                                  // the lowest face among those at d2
    int par;                                   // bit k: the parity along axis k
};
TGS_SDF_HD Best best_init() { return {INFINITY, {0.0, 0.0, 0.0}, -1, 0}; }
TGS_SDF_HD void best_distance(Best& b, D3 p, D3 v0, D3 v1, D3 v2, int face)
{
    const D3 c = closest_on_triangle(p, v0, v1, v2);
    const double d2 = dist2(p, c);
    if (d2 < b.d2 || (d2 == b.d2 && face < b.face)) { b.d2 = d2; b.c = c; b.face = face; }
}
TGS_SDF_HD void best_parity(Best& b, D3 p, D3 v0, D3 v1, D3 v2, int i0, int i1, int i2)
{
    b.par ^= crossing<0>(p, v0, v1, v2, i0, i1, i2) | (crossing<1>(p, v0, v1, v2, i0, i1, i2) << 1) | (crossing<2>(p, v0, v1, v2, i0, i1, i2) << 2);
}

// the outputs of one point; each pointer may be NULL.  inside: at least two odd parities, or d == 0.
TGS_SDF_HD void write_point(const Best& b, bool finite, long long n, float* out_sdf, int32_t* out_face, float* out_closest, uint8_t* out_inside)
{
    const bool found = finite && b.face >= 0;
    const float d = found ? (float)sqrt(b.d2) : NAN;
    const bool in = found && (b.d2 == 0.0 || ((b.par & 1) + ((b.par >> 1) & 1) + ((b.par >> 2) & 1)) >= 2);
    if (out_sdf) out_sdf[n] = !found ? NAN : (b.d2 == 0.0 ? 0.0f : (in ? d : -d));
    if (out_face) out_face[n] = found ? b.face : -1;
    if (out_closest) { out_closest[3 * n] = found ? (float)b.c.x : NAN; out_closest[3 * n + 1] = found ? (float)b.c.y : NAN; out_closest[3 * n + 2] = found ? (float)b.c.z : NAN; }
    if (out_inside) out_inside[n] = in ? 1 : 0;
}

// ---- mode 1: every face, in the caller's order ------------------------------------------------------------------------------------------
template <typename Index>
TGS_SDF_HD void point_brute(int V, int F, const float* vertices, const Index* faces, const float* points, long long n, bool sign,
                            float* out_sdf, int32_t* out_face, float* out_closest, uint8_t* out_inside)
{
    const bool finite = finite3(points + 3 * n);
    Best b = best_init();
    if (finite) {
        const D3 p = load3(points + 3 * n);
        for (int f = 0; f < F; ++f) {
            const long long i0 = (long long)faces[3 * (size_t)f], i1 = (long long)faces[3 * (size_t)f + 1], i2 = (long long)faces[3 * (size_t)f + 2];
            if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) continue;         // refused at build time; never read through
            const D3 v0 = load3(vertices + 3 * i0), v1 = load3(vertices + 3 * i1), v2 = load3(vertices + 3 * i2);
            best_distance(b, p, v0, v1, v2, f);
            if (sign) best_parity(b, p, v0, v1, v2, (int)i0, (int)i1, (int)i2);
        }
    }
    write_point(b, finite, n, out_sdf, out_face, out_closest, out_inside);
}

// ---- mode 0: the tree, without a stack ---------------------------------------------------------------------------------------------------
TGS_SDF_HD void leaf_range(const Node& nd, int F, int& first, int& count)
{
    first = nd.leaf >> 3; count = nd.leaf & 7;
    if (first < 0 || count > LEAF_FACES || first + count > F) count = 0;                         // a corrupt word reads nothing
}
TGS_SDF_HD void leaf_distance(Best& b, D3 p, const Record* rec, int first, int count)
{
    for (int r = first; r < first + count; ++r)
        best_distance(b, p, load3(rec[r].v), load3(rec[r].v + 3), load3(rec[r].v + 6), rec[r].face);
}

TGS_SDF_HD void point_tree(const void* tree, int F, const float* points, long long n, bool sign, float* out_sdf, int32_t* out_face, float* out_closest, uint8_t* out_inside)
{
    const Header* h = (const Header*)tree;
    const Node* nodes = tree_nodes(tree);
    const Record* rec = tree_records(tree, (size_t)F);
    const bool finite = finite3(points + 3 * n) && h->magic == MAGIC && h->n_faces == (uint32_t)F;
    const int N = h->n_nodes <= 2u * (uint32_t)F ? (int)h->n_nodes : 0;
    Best b = best_init();
    if (finite && N > 0) {
        const D3 p = load3(points + 3 * n);
        int first, count;
        // 1. down to the leaf behind the nearer box at every level: a tight bound to start with.  At most MAX_DEPTH + 1 nodes.
        int i = 0;
        for (int level = 0; level <= MAX_DEPTH && i >= 0 && i < N; ++level) {
            const Node nd = nodes[i];
            if (nd.leaf >= 0) { leaf_range(nd, F, first, count); leaf_distance(b, p, rec, first, count); break; }
            const int l = i + 1, r = l < N ? nodes[l].skip : N;
            i = (r > l && r < N && box_lower_bound(p, nodes[r]) < box_lower_bound(p, nodes[l])) ? r : l;
        }
        // 2. the whole tree in depth-first order: into a box whose lower bound is not strictly greater than the best so far (ties are visited),
        // past its subtree otherwise.  The node index only grows and is bounded by the node count, whatever the tree holds.
        for (i = 0; i < N;) {
            const Node nd = nodes[i];
            int next = i + 1;
            if (box_lower_bound(p, nd) > b.d2) next = nd.skip;
            else if (nd.leaf >= 0) { leaf_range(nd, F, first, count); leaf_distance(b, p, rec, first, count); }
            i = next > i ? next : i + 1;
        }
        // 3. the three parities in one more walk: into a box that a ray along some axis may cross
        for (i = 0; sign && i < N;) {
            const Node nd = nodes[i];
            int next = i + 1;
            if (!box_ray_axes(p, nd)) next = nd.skip;
            else if (nd.leaf >= 0) {
                leaf_range(nd, F, first, count);
                for (int r = first; r < first + count; ++r)
                    best_parity(b, p, load3(rec[r].v), load3(rec[r].v + 3), load3(rec[r].v + 6), rec[r].idx[0], rec[r].idx[1], rec[r].idx[2]);
            }
            i = next > i ? next : i + 1;
        }
    }
    write_point(b, finite, n, out_sdf, out_face, out_closest, out_inside);
}

// ---- the host build ------------------------------------------------------------------------------------------------------------------------
// Median splits of the face centroids along the longest axis of their extent, the lower half (by key, then by face number) to the left; a leaf
// holds its faces in ascending order.  No device call.  -> NULL, or what is wrong with the arguments.
struct Builder {
    const float* vert; const void* faces; bool is64; int F;
    Node* nodes; Record* rec; std::vector<int> order; std::vector<float> cen;
    int n_nodes = 0, n_rec = 0, depth = 0; float pad = 0.0f;

    long long index(int f, int k) const { return is64 ? (long long)((const int64_t*)faces)[3 * (size_t)f + k] : (long long)((const int32_t*)faces)[3 * (size_t)f + k]; }
    static float down(double x) { return nextafterf((float)x, -INFINITY); }        // (float)x is within half an ulp of x: one more step is below it
    static float up(double x) { return nextafterf((float)x, INFINITY); }

    int build(int lo, int hi, int level)
    {
        const int i = n_nodes++;
        Node& nd = nodes[i];
        if (level > depth) depth = level;
        if (hi - lo <= LEAF_FACES || level >= MAX_DEPTH) {
            if (hi - lo > LEAF_FACES) return -1;
            std::sort(order.begin() + lo, order.begin() + hi);
            nd.leaf = 8 * n_rec + (hi - lo);
            float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int k = lo; k < hi; ++k) {
                Record& r = rec[n_rec++];
                r.face = order[k];
                for (int c = 0; c < 3; ++c) {
                    r.idx[c] = (int32_t)index(order[k], c);
                    for (int a = 0; a < 3; ++a) {
                        const float x = vert[3 * (size_t)r.idx[c] + a];
                        r.v[3 * c + a] = x; mn[a] = x < mn[a] ? x : mn[a]; mx[a] = x > mx[a] ? x : mx[a];
                    }
                }
            }
            for (int a = 0; a < 3; ++a) { nd.lo[a] = down((double)mn[a] - (double)pad); nd.hi[a] = up((double)mx[a] + (double)pad); }
            nd.skip = n_nodes;
            return i;
        }
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = lo; k < hi; ++k)
            for (int a = 0; a < 3; ++a) { const float x = cen[3 * (size_t)order[k] + a]; mn[a] = x < mn[a] ? x : mn[a]; mx[a] = x > mx[a] ? x : mx[a]; }
        int ax = 0;
        if (mx[1] - mn[1] > mx[ax] - mn[ax]) ax = 1;
        if (mx[2] - mn[2] > mx[ax] - mn[ax]) ax = 2;
        const int mid = lo + (hi - lo + 1) / 2;
        const float* c = cen.data();
        std::nth_element(order.begin() + lo, order.begin() + mid, order.begin() + hi, [c, ax](int x, int y) {
            const float kx = c[3 * (size_t)x + ax], ky = c[3 * (size_t)y + ax];
            return kx < ky || (kx == ky && x < y);
        });
        const int l = build(lo, mid, level + 1);
        const int r = l < 0 ? -1 : build(mid, hi, level + 1);
        if (r < 0) return -1;
        Node& me = nodes[i];
        for (int a = 0; a < 3; ++a) { me.lo[a] = nodes[l].lo[a] < nodes[r].lo[a] ? nodes[l].lo[a] : nodes[r].lo[a]; me.hi[a] = nodes[l].hi[a] > nodes[r].hi[a] ? nodes[l].hi[a] : nodes[r].hi[a]; }
        me.skip = n_nodes; me.leaf = -1;
        return i;
    }
};

inline const char* build_tree(int V, int F, const float* vertices, const void* faces, int faces_is_int64, void* tree, size_t bytes)
{
    if (V < 1 || F < 1 || !vertices || !faces || !tree || (faces_is_int64 != 0 && faces_is_int64 != 1))
        return "V >= 1, F >= 1, faces_is_int64 in {0, 1} and non-NULL vertices / faces / tree required";
    if (F > MAX_FACES) return "F above the limit of 2^28 - 1 faces";
    if (bytes < tree_bytes((size_t)F)) return "tree smaller than tgs_meshsdf_tree_bytes(F)";
    float big = 0.0f;
    for (size_t k = 0; k < 3 * (size_t)V; ++k) {
        if (!finite1(vertices[k])) return "a vertex coordinate is not finite";
        big = fabsf(vertices[k]) > big ? fabsf(vertices[k]) : big;
    }
    Builder b;
    b.vert = vertices; b.faces = faces; b.is64 = faces_is_int64 != 0; b.F = F;
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k)
            if (b.index(f, k) < 0 || b.index(f, k) >= V) return "faces holds a vertex index outside [0, V)";
    memset(tree, 0, tree_bytes((size_t)F));                                        // two builds give the same bytes, the unused tail included
    b.nodes = (Node*)tree_nodes(tree); b.rec = (Record*)tree_records(tree, (size_t)F);
    b.pad = (float)((double)big * 0x1p-20);
    b.order.resize((size_t)F); b.cen.resize(3 * (size_t)F);
    for (int f = 0; f < F; ++f) {
        b.order[(size_t)f] = f;
        for (int a = 0; a < 3; ++a)
            b.cen[3 * (size_t)f + a] = (float)((((double)vertices[3 * b.index(f, 0) + a] + (double)vertices[3 * b.index(f, 1) + a]) + (double)vertices[3 * b.index(f, 2) + a]) / 3.0);
    }
    if (b.build(0, F, 0) < 0 || b.n_rec != F || b.n_nodes > 2 * F || b.depth > MAX_DEPTH) return "the tree's depth bound does not hold";
    Header* h = (Header*)tree;
    h->magic = MAGIC; h->n_faces = (uint32_t)F; h->n_nodes = (uint32_t)b.n_nodes; h->depth = (uint32_t)b.depth; h->leaf_faces = LEAF_FACES;
    return nullptr;
}

// what every query checks before it walks -> NULL or the message
inline const char* check_query(const void* tree, size_t bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, long long N, const float* points, int mode)
{
    if (V < 1 || F < 1 || F > MAX_FACES || N < 0 || !tree || !vertices || !faces || (N > 0 && !points) || (faces_is_int64 != 0 && faces_is_int64 != 1))
        return "V >= 1, 1 <= F <= 2^28 - 1, N >= 0, faces_is_int64 in {0, 1} and non-NULL tree / vertices / faces / points required";
    if (mode != 0 && mode != 1) return "mode is 0 (the tree) or 1 (every face)";
    if (bytes < tree_bytes((size_t)F)) return "tree smaller than tgs_meshsdf_tree_bytes(F)";
    return nullptr;
}

inline const char* query_host(const void* tree, size_t bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, long long N, const float* points, int mode,
                              float* out_sdf, int32_t* out_face, float* out_closest, uint8_t* out_inside)
{
    if (const char* bad = check_query(tree, bytes, V, F, vertices, faces, faces_is_int64, N, points, mode)) return bad;
    const Header* h = (const Header*)tree;
    if (h->magic != MAGIC || h->n_faces != (uint32_t)F) return "tree was not built by tgs_meshsdf_build for this F";
    const bool sign = out_sdf || out_inside;
    for (long long n = 0; n < N; ++n) {
        if (mode == 0) point_tree(tree, F, points, n, sign, out_sdf, out_face, out_closest, out_inside);
        else if (faces_is_int64) point_brute(V, F, vertices, (const int64_t*)faces, points, n, sign, out_sdf, out_face, out_closest, out_inside);
        else point_brute(V, F, vertices, (const int32_t*)faces, points, n, sign, out_sdf, out_face, out_closest, out_inside);
    }
    return nullptr;
}

}  // namespace msdf
}  // namespace tgs
#endif  // TGS_MESH_SDF_HPP
