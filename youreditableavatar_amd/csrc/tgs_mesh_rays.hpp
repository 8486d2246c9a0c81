// tgs_mesh_rays.hpp -- rays against a triangle mesh: the per-pair functions (ray against face, ray against box) and the two walks, shared by the
// device kernels (tgs_mesh_rays.hip), the host twins (tgs_meshrays_cast_host, tgs_meshrays_occluded_host) and the stand-alone host check
// (tools/mesh_rays_host_check.cpp).  Plain C++17, host and device.  The tree is the mesh signed distance's (tgs_mesh_sdf.hpp: Node, Record, the
// accessors, build_tree), byte for byte: a mesh that has one needs no second build.  include/tgs_raster.h ("mesh ray casting") has the rules in
// full; tests/mesh_rays_ref.py restates them in numpy float64.
//
// All arithmetic is in double on the float32 inputs and is compiled without contraction (the pragma of tgs_mesh_sdf.hpp, and -ffp-contract=off on
// the file), so the host build, the device build and the restatement evaluate the same expressions.  No per-lane array: an axis is chosen with
// selects (pick), never with a runtime index.
#ifndef TGS_MESH_RAYS_HPP
#define TGS_MESH_RAYS_HPP

#include "tgs_mesh_sdf.hpp"

namespace tgs {
namespace mrays {

using msdf::D3;
using msdf::Header;
using msdf::Node;
using msdf::Record;

TGS_SDF_HD double pick(D3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }
TGS_SDF_HD bool finite_d(double x) { return x - x == 0.0; }

// ---- the ray: validity, the axis permutation and the shear (Woop, Benthin, Wald: Watertight Ray/Triangle Intersection, JCGT 2013) --------
struct Ray {
    D3 o, d;
    int kx, ky, kz;                            // kz: the axis of the largest |d_k| (the lowest on a tie); kx, ky: the next two in cyclic order, swapped when d[kz] < 0
    double Sx, Sy, Sz;
    bool valid;                                // six finite components and d != (0, 0, 0)
};
TGS_SDF_HD Ray ray_setup(const float* r)
{
    Ray y;
    y.valid = msdf::finite3(r) && msdf::finite3(r + 3) && !(r[3] == 0.0f && r[4] == 0.0f && r[5] == 0.0f);
    y.o = msdf::load3(r); y.d = msdf::load3(r + 3);
    const double ax = fabs(y.d.x), ay = fabs(y.d.y), az = fabs(y.d.z);
    int kz = 0;
    double m = ax;
    if (ay > m) { kz = 1; m = ay; }
    if (az > m) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dz = y.valid ? pick(y.d, kz) : 1.0;                                           // (an invalid ray divides nothing by zero; it is never walked)
    if (dz < 0.0) { const int s = kx; kx = ky; ky = s; }
    y.kx = kx; y.ky = ky; y.kz = kz;
    y.Sx = pick(y.d, kx) / dz; y.Sy = pick(y.d, ky) / dz; y.Sz = 1.0 / dz;
    return y;
}
// a vertex as the ray sees it: a function of the vertex and the ray alone, not of the face
TGS_SDF_HD D3 shear(const Ray& y, D3 P)
{
    const D3 A = msdf::sub(P, y.o);
    const double az = pick(A, y.kz);
    return {pick(A, y.kx) - y.Sx * az, pick(A, y.ky) - y.Sy * az, y.Sz * az};
}
TGS_SDF_HD D3 face_cross(D3 v0, D3 v1, D3 v2)
{
    const D3 a = msdf::sub(v1, v0), b = msdf::sub(v2, v0);
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// ---- pair function 1: the ray against a face -> a hit?  t, and the weights V, W and det of the uvs ----------------------------------------
TGS_SDF_HD bool ray_face(const Ray& y, D3 v0, D3 v1, D3 v2, double& t, double& V, double& W, double& det)
{
    const D3 A = shear(y, v0), B = shear(y, v1), C = shear(y, v2);
    const double U = C.x * B.y - C.y * B.x;
    V = A.x * C.y - A.y * C.x;
    W = B.x * A.y - B.y * A.x;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;      // exact zeros belong to both sides
    det = (U + V) + W;
    if (det == 0.0) return false;
    t = ((U * A.z + V * B.z) + W * C.z) / det;
    if (!(t >= 0.0) || !finite_d(t)) return false;
    const D3 n = face_cross(v0, v1, v2);                                                       // a face without a normal is no hit, whatever det rounded to
    return !(n.x == 0.0 && n.y == 0.0 && n.z == 0.0);
}

// ---- pair function 2: the ray against a box, for 0 <= t <= far.  Ties are entered. ----------------------------------------------------------
TGS_SDF_HD bool slab(double o, double d, double lo, double hi, double& t0, double& t1)
{
    if (d == 0.0) return lo <= o && o <= hi;
    const double a = (lo - o) / d, b = (hi - o) / d;
    const double en = a < b ? a : b, ex = a < b ? b : a;
    t0 = en > t0 ? en : t0;
    t1 = ex < t1 ? ex : t1;
    return true;
}
TGS_SDF_HD bool ray_box(const Ray& y, const Node& n, double far)
{
    double t0 = 0.0, t1 = far;
    const bool in = slab(y.o.x, y.d.x, (double)n.lo[0], (double)n.hi[0], t0, t1) && slab(y.o.y, y.d.y, (double)n.lo[1], (double)n.hi[1], t0, t1) &&
                    slab(y.o.z, y.d.z, (double)n.lo[2], (double)n.hi[2], t0, t1);
    return in && t0 <= t1;
}

// ---- one ray's state ------------------------------------------------------------------------------------------------------------------------
struct Best {
    double t, u, v;                            // the least t so far and that face's uv
    int face;                                  // the lowest face among those at t
    int slot;                                  // where its vertices are: the face's row (mode 1) or its record (mode 0)
};
TGS_SDF_HD Best best_init() { return {INFINITY, 0.0, 0.0, -1, -1}; }
TGS_SDF_HD void best_face(Best& b, const Ray& y, D3 v0, D3 v1, D3 v2, int face, int slot)
{
    double t, V, W, det;
    if (!ray_face(y, v0, v1, v2, t, V, W, det)) return;
    if (t < b.t || (t == b.t && face < b.face)) { b.t = t; b.u = V / det; b.v = W / det; b.face = face; b.slot = slot; }
}
TGS_SDF_HD bool face_between(const Ray& y, D3 v0, D3 v1, D3 v2, double tnear, double tfar)
{
    double t, V, W, det;
    return ray_face(y, v0, v1, v2, t, V, W, det) && tnear <= t && t <= tfar;
}

// the outputs of one ray; each pointer may be NULL.  (v0, v1, v2): the vertices of b.face, read only on a hit.  A hit face outside [0, F) -- a
// corrupt record -- is a miss row: out_hit_faces is never written out of bounds.
TGS_SDF_HD void write_ray(const Best& b, int F, D3 v0, D3 v1, D3 v2, long long n, float* out_t, int32_t* out_face, int32_t* out_geometry, float* out_uv, float* out_normal,
                          uint8_t* out_hit_faces)
{
    const bool hit = b.face >= 0 && b.face < F;
    if (out_t) out_t[n] = hit ? (float)b.t : INFINITY;
    if (out_face) out_face[n] = hit ? b.face : -1;
    if (out_geometry) out_geometry[n] = hit ? 0 : -1;
    if (out_uv) { out_uv[2 * n] = hit ? (float)b.u : 0.0f; out_uv[2 * n + 1] = hit ? (float)b.v : 0.0f; }
    if (out_normal) {
        D3 c = {0.0, 0.0, 0.0};
        if (hit) {
            const D3 nn = face_cross(v0, v1, v2);
            const double len = sqrt(msdf::dot(nn, nn));
            c = {nn.x / len, nn.y / len, nn.z / len};
        }
        out_normal[3 * n] = (float)c.x; out_normal[3 * n + 1] = (float)c.y; out_normal[3 * n + 2] = (float)c.z;
    }
    if (out_hit_faces && hit) out_hit_faces[b.face] = 1;                                         // several lanes may store the same value
}

template <typename Index>
TGS_SDF_HD bool face_vertices(int V, const float* vertices, const Index* faces, int f, D3& v0, D3& v1, D3& v2)
{
    const long long i0 = (long long)faces[3 * (size_t)f], i1 = (long long)faces[3 * (size_t)f + 1], i2 = (long long)faces[3 * (size_t)f + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;                  // refused at build time; never read through
    v0 = msdf::load3(vertices + 3 * i0); v1 = msdf::load3(vertices + 3 * i1); v2 = msdf::load3(vertices + 3 * i2);
    return true;
}
TGS_SDF_HD void record_vertices(const Record& r, D3& v0, D3& v1, D3& v2) { v0 = msdf::load3(r.v); v1 = msdf::load3(r.v + 3); v2 = msdf::load3(r.v + 6); }

// ---- mode 1: every face, in the caller's order -----------------------------------------------------------------------------------------------
template <typename Index>
TGS_SDF_HD void cast_brute(int V, int F, const float* vertices, const Index* faces, const float* rays, long long n, float* out_t, int32_t* out_face, int32_t* out_geometry,
                           float* out_uv, float* out_normal, uint8_t* out_hit_faces)
{
    const Ray y = ray_setup(rays + 6 * n);
    Best b = best_init();
    D3 v0 = {0.0, 0.0, 0.0}, v1 = v0, v2 = v0;
    if (y.valid) {
        for (int f = 0; f < F; ++f)
            if (face_vertices(V, vertices, faces, f, v0, v1, v2)) best_face(b, y, v0, v1, v2, f, f);
        if (b.face >= 0) face_vertices(V, vertices, faces, b.slot, v0, v1, v2);
    }
    write_ray(b, F, v0, v1, v2, n, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
}
template <typename Index>
TGS_SDF_HD void occluded_brute(int V, int F, const float* vertices, const Index* faces, const float* rays, long long n, double tnear, double tfar, uint8_t* out_occluded)
{
    const Ray y = ray_setup(rays + 6 * n);
    bool found = false;
    D3 v0, v1, v2;
    for (int f = 0; y.valid && !found && f < F; ++f)
        found = face_vertices(V, vertices, faces, f, v0, v1, v2) && face_between(y, v0, v1, v2, tnear, tfar);
    out_occluded[n] = found ? 1 : 0;
}

// ---- mode 0: the tree in depth-first order with the skip links, without a stack ------------------------------------------------------------------
// The node index only grows and is bounded by the node count, whatever the tree holds; a leaf word that does not fit reads nothing (leaf_range).
TGS_SDF_HD int tree_nodes_checked(const void* tree, int F)
{
    const Header* h = (const Header*)tree;
    return (h->magic == msdf::MAGIC && h->n_faces == (uint32_t)F && h->n_nodes <= 2u * (uint32_t)F) ? (int)h->n_nodes : 0;
}
TGS_SDF_HD void cast_tree(const void* tree, int F, const float* rays, long long n, float* out_t, int32_t* out_face, int32_t* out_geometry, float* out_uv, float* out_normal,
                          uint8_t* out_hit_faces)
{
    const Node* nodes = msdf::tree_nodes(tree);
    const Record* rec = msdf::tree_records(tree, (size_t)F);
    const int N = tree_nodes_checked(tree, F);
    const Ray y = ray_setup(rays + 6 * n);
    Best b = best_init();
    D3 v0 = {0.0, 0.0, 0.0}, v1 = v0, v2 = v0;
    if (y.valid) {
        for (int i = 0; i < N;) {
            const Node nd = nodes[i];
            int next = i + 1;
            if (!ray_box(y, nd, b.t)) next = nd.skip;
            else if (nd.leaf >= 0) {
                int first, count;
                msdf::leaf_range(nd, F, first, count);
                for (int r = first; r < first + count; ++r) { record_vertices(rec[r], v0, v1, v2); best_face(b, y, v0, v1, v2, rec[r].face, r); }
            }
            i = next > i ? next : i + 1;
        }
        if (b.face >= 0) record_vertices(rec[b.slot], v0, v1, v2);
    }
    write_ray(b, F, v0, v1, v2, n, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
}
TGS_SDF_HD void occluded_tree(const void* tree, int F, const float* rays, long long n, double tnear, double tfar, uint8_t* out_occluded)
{
    const Node* nodes = msdf::tree_nodes(tree);
    const Record* rec = msdf::tree_records(tree, (size_t)F);
    const int N = tree_nodes_checked(tree, F);
    const Ray y = ray_setup(rays + 6 * n);
    bool found = false;
    for (int i = 0; y.valid && !found && i < N;) {
        const Node nd = nodes[i];
        int next = i + 1;
        if (!ray_box(y, nd, tfar)) next = nd.skip;
        else if (nd.leaf >= 0) {
            int first, count;
            msdf::leaf_range(nd, F, first, count);
            D3 v0, v1, v2;
            for (int r = first; !found && r < first + count; ++r) { record_vertices(rec[r], v0, v1, v2); found = face_between(y, v0, v1, v2, tnear, tfar); }
        }
        i = next > i ? next : i + 1;
    }
    out_occluded[n] = found ? 1 : 0;
}

// ---- what every call checks before it walks -> NULL or the message ---------------------------------------------------------------------------
inline const char* check_cast(const void* tree, size_t bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, long long N, const float* rays, int mode)
{
    if (V < 1 || F < 1 || F > msdf::MAX_FACES || N < 0 || !tree || !vertices || !faces || (N > 0 && !rays) || (faces_is_int64 != 0 && faces_is_int64 != 1))
        return "V >= 1, 1 <= F <= 2^28 - 1, N >= 0, faces_is_int64 in {0, 1} and non-NULL tree / vertices / faces / rays required";
    if (mode != 0 && mode != 1) return "mode is 0 (the tree) or 1 (every face)";
    if (bytes < msdf::tree_bytes((size_t)F)) return "tree smaller than tgs_meshsdf_tree_bytes(F)";
    return nullptr;
}
inline const char* check_occluded(const void* tree, size_t bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, long long N, const float* rays,
                                  float tnear, float tfar, int mode, const uint8_t* out_occluded)
{
    if (const char* bad = check_cast(tree, bytes, V, F, vertices, faces, faces_is_int64, N, rays, mode)) return bad;
    if (!(tnear <= tfar)) return "tnear <= tfar required, neither a NaN";
    if (N > 0 && !out_occluded) return "non-NULL out_occluded required";
    return nullptr;
}

inline const char* cast_host(const void* tree, size_t bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, long long N, const float* rays, int mode,
                             float* out_t, int32_t* out_face, int32_t* out_geometry, float* out_uv, float* out_normal, uint8_t* out_hit_faces)
{
    if (const char* bad = check_cast(tree, bytes, V, F, vertices, faces, faces_is_int64, N, rays, mode)) return bad;
    for (long long n = 0; n < N; ++n) {
        if (mode == 0) cast_tree(tree, F, rays, n, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
        else if (faces_is_int64) cast_brute(V, F, vertices, (const int64_t*)faces, rays, n, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
        else cast_brute(V, F, vertices, (const int32_t*)faces, rays, n, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
    }
    return nullptr;
}
inline const char* occluded_host(const void* tree, size_t bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, long long N, const float* rays,
                                 float tnear, float tfar, int mode, uint8_t* out_occluded)
{
    if (const char* bad = check_occluded(tree, bytes, V, F, vertices, faces, faces_is_int64, N, rays, tnear, tfar, mode, out_occluded)) return bad;
    for (long long n = 0; n < N; ++n) {
        if (mode == 0) occluded_tree(tree, F, rays, n, (double)tnear, (double)tfar, out_occluded);
        else if (faces_is_int64) occluded_brute(V, F, vertices, (const int64_t*)faces, rays, n, (double)tnear, (double)tfar, out_occluded);
        else occluded_brute(V, F, vertices, (const int32_t*)faces, rays, n, (double)tnear, (double)tfar, out_occluded);
    }
    return nullptr;
}

}  // namespace mrays
}  // namespace tgs
#endif  // TGS_MESH_RAYS_HPP
