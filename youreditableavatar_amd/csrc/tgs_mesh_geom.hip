// tgs_mesh_geom.hip -- what the geometry stage computes on a fresh mesh between marching tetrahedra and the mesh rasterizer: vertex normals
// (tetgs_spatial/models/renderers/nvdiff_rasterize_utils.py :12-35, :37-70; models/mesh.py :136-162), the distinct edges (mesh.py :261-273), the
// normal-consistency loss (:275-280) and the uniform-Laplacian loss (:282-315), forward and backward, for gfx950.  Plain HIP, wave64.  Integer
// atomics only (the dedupe's CAS, integer counters and cursors); no float atomics anywhere and no atomics at all on gradient memory; every output
// position comes from a prefix sum or a sorted run, so two runs give the same bits.  include/tgs_raster.h ("mesh geometry") has the rules in
// full; tests/mesh_geom_ref.py restates them.
//
// The topology is built once per mesh, in two calls around one read-back (E and the index flag):
//   tgs_meshgeom_topology_count  k_mg_count (one lane per face: the range check, one count per corner's vertex, the three sides into the edge
//                                 set of tgs_edge_set.hpp; whoever claims a free slot adds one to the count of the side's min vertex and of
//                                 its max vertex), three scans over V + 1 (tgs_runs.hpp) -> counts[0] = E.
//   tgs_meshgeom_topology_fill   k_mg_inc_fill (3 * face + corner into the vertex's run, through a cursor), k_mg_sort_u32 (one lane per vertex
//                                 sorts its run), k_edge_fill and k_edge_sort (tgs_edge_set.hpp: the edges are now in ascending (min, max)
//                                 order whatever the cursors did), k_mg_max_fill (edge numbers by max vertex), k_mg_sort_u32 again.
// After the fill the three offset arrays hold the ENDS of the runs: vertex v's run is run_bounds(end, v, n) of tgs_runs.hpp.
// Every later call is a gather: one lane per vertex over its run(s), or one lane per face / per edge; sums in double, in run order, rounded to
// fp32 once.  The two losses reduce per workgroup in double (a fixed shuffle tree) and one workgroup adds the partial sums in a fixed order.
#include "tgs_edge_set.hpp"                                             // the edge set; with it tgs_runs.hpp: the scans, the run bounds and the run sort

namespace tgs {

constexpr long long MG_MAX_FACES = 1431655765ll;                        // 3 F < 2^32: incidence entries and edge numbers are 32-bit
constexpr double MG_NORMAL_EPS = 1e-20;                                 // the reference's threshold on the squared length
constexpr double MG_COSINE_EPS = 1e-8;                                  // torch.cosine_similarity's default eps

struct MgWork {
    uint32_t* scan;                       // scratch of the scans over V + 1
    double* partial;                      // [ceil(max(V, 3 F) / 256) + 1] the workgroups' sums of a loss
};
__host__ __device__ inline size_t mg_carve(MgWork& w, char* base, size_t V, size_t F)
{
    char* p = base;
    const size_t big = V > 3 * F ? V : 3 * F;
    carve(p, w.scan, run_scan_scratch(V + 1)); carve(p, w.partial, run_blocks(big) + 1);
    return (size_t)(p - base) + 256;
}
struct MgGradWork {
    double* g_sum;                        // [V,3] the upstream taken through the normalization: the gradient of the vertex's summed normal
    double* g_face;                       // [F,3] the gradient of the face's normal: its three corners' g_sum added
};
__host__ __device__ inline size_t mg_grad_carve(MgGradWork& w, char* base, size_t V, size_t F)
{
    char* p = base;
    carve(p, w.g_sum, 3 * V + 1); carve(p, w.g_face, 3 * F + 1);
    return (size_t)(p - base) + 256;
}
__host__ __device__ inline size_t mg_table_capacity(size_t F)
{
    size_t cap = 64;                                                    // a power of two >= 6 F: load <= 1/2 with 3 F sides
    while (cap < 6 * F) cap <<= 1;
    return cap;
}

// ---- the topology ----
template <typename Idx>
__device__ __forceinline__ bool mg_load_face(const Idx* __restrict__ faces, size_t f, int V, long long i[3])
{
    i[0] = (long long)faces[3 * f]; i[1] = (long long)faces[3 * f + 1]; i[2] = (long long)faces[3 * f + 2];
    return (unsigned long long)i[0] < (unsigned long long)V && (unsigned long long)i[1] < (unsigned long long)V && (unsigned long long)i[2] < (unsigned long long)V;
}

template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_count(int V, int F, const Idx* __restrict__ faces, uint32_t* __restrict__ inc_end, uint32_t* __restrict__ edge_end,
                                                       uint32_t* __restrict__ max_end, size_t cap, unsigned long long* __restrict__ keys, long long* __restrict__ counts)
{
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (f >= (size_t)F) return;
    long long i[3];
    if (!mg_load_face(faces, f, V, i)) {
        atomicOr((unsigned long long*)&counts[1], 1ull);                 // refused by the caller after the read-back; the face is left out here
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) atomicAdd(&inc_end[i[c]], 1u);
    if (!keys) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const long long x = i[c], y = i[c == 2 ? 0 : c + 1];
        const long long a = x < y ? x : y, b = x < y ? y : x;
        bool claimed;
        edge_insert(keys, cap, edge_key(a, b), claimed);
        if (claimed) { atomicAdd(&edge_end[a], 1u); atomicAdd(&max_end[b], 1u); }
    }
}

template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_inc_fill(int V, int F, const Idx* __restrict__ faces, uint32_t* __restrict__ inc_end, uint32_t* __restrict__ inc)
{
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (f >= (size_t)F) return;
    long long i[3];
    if (!mg_load_face(faces, f, V, i)) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const size_t p = atomicAdd(&inc_end[i[c]], 1u);                  // the cursor: inc_end[v] ends at the start of v + 1's run
        if (p < 3 * (size_t)F) inc[p] = (uint32_t)(3 * f + c);
    }
}

// end[v] is now the END of v's run (the start of v + 1's); one lane sorts a vertex's run ascending
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_sort_u32(int V, size_t n, const uint32_t* __restrict__ end, uint32_t* __restrict__ list)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= (size_t)V) return;
    const Run run = run_bounds(end, v, n);
    run_sort(list, 1, (long long)run.lo, (long long)run.hi);
}

__global__ __launch_bounds__(RUN_BLOCK) void k_mg_max_fill(int V, long long E, const long long* __restrict__ edges, uint32_t* __restrict__ max_end, uint32_t* __restrict__ max_list)
{
    const long long e = (long long)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (e >= E) return;
    const long long b = edges[2 * e + 1];
    if ((unsigned long long)b >= (unsigned long long)V) return;
    const long long p = atomicAdd(&max_end[b], 1u);
    if (p < E) max_list[p] = (uint32_t)e;
}

__device__ __forceinline__ void mg_row(const float* __restrict__ x, long long v, double r[3])
{
    r[0] = x[3 * v]; r[1] = x[3 * v + 1]; r[2] = x[3 * v + 2];
}
__device__ __forceinline__ void mg_cross(const double a[3], const double b[3], double r[3])
{
    r[0] = a[1] * b[2] - a[2] * b[1]; r[1] = a[2] * b[0] - a[0] * b[2]; r[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- vertex normals ----
// the sum of the face normals cross(v1 - v0, v2 - v0) over v's incidence run, in double, in run order
template <typename Idx>
__device__ __forceinline__ void mg_normal_sum(int V, int F, const float* __restrict__ v_pos, const Idx* __restrict__ faces, const uint32_t* __restrict__ inc_end,
                                              const uint32_t* __restrict__ inc, size_t v, double s[3])
{
    s[0] = s[1] = s[2] = 0.0;
    const Run run = run_bounds(inc_end, v, 3 * (size_t)F);
    for (size_t k = run.lo; k < run.hi; k++) {
        const size_t f = inc[k] / 3u;
        long long i[3];
        if (f >= (size_t)F || !mg_load_face(faces, f, V, i)) continue;
        double p0[3], p1[3], p2[3], e1[3], e2[3], n[3];
        mg_row(v_pos, i[0], p0); mg_row(v_pos, i[1], p1); mg_row(v_pos, i[2], p2);
#pragma unroll
        for (int d = 0; d < 3; d++) { e1[d] = p1[d] - p0[d]; e2[d] = p2[d] - p0[d]; }
        mg_cross(e1, e2, n);
        s[0] += n[0]; s[1] += n[1]; s[2] += n[2];
    }
}

template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_normals(int V, int F, const float* __restrict__ v_pos, const Idx* __restrict__ faces, const uint32_t* __restrict__ inc_end,
                                                         const uint32_t* __restrict__ inc, float* __restrict__ v_nrm)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= (size_t)V) return;
    double s[3];
    mg_normal_sum(V, F, v_pos, faces, inc_end, inc, v, s);
    const double sq = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
    float n[3] = {0.f, 0.f, 1.f};
    if (sq > MG_NORMAL_EPS) {                                           // false for a NaN: the default row
        const double len = sqrt(sq);
        n[0] = (float)(s[0] / len); n[1] = (float)(s[1] / len); n[2] = (float)(s[2] / len);
    }
    v_nrm[3 * v] = n[0]; v_nrm[3 * v + 1] = n[1]; v_nrm[3 * v + 2] = n[2];
}

// the upstream through the normalization n = s / |s|: g_sum = (g - n (n . g)) / |s|, an exact zero for a default row
template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_normals_bwd_vertex(int V, int F, const float* __restrict__ v_pos, const Idx* __restrict__ faces,
                                                                    const uint32_t* __restrict__ inc_end, const uint32_t* __restrict__ inc, const float* __restrict__ g_nrm,
                                                                    double* __restrict__ g_sum)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= (size_t)V) return;
    double s[3], out[3] = {0.0, 0.0, 0.0};
    mg_normal_sum(V, F, v_pos, faces, inc_end, inc, v, s);
    const double sq = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
    if (sq > MG_NORMAL_EPS) {
        const double len = sqrt(sq);
        double g[3], n[3];
        mg_row(g_nrm, (long long)v, g);
        n[0] = s[0] / len; n[1] = s[1] / len; n[2] = s[2] / len;
        const double dot = n[0] * g[0] + n[1] * g[1] + n[2] * g[2];
#pragma unroll
        for (int d = 0; d < 3; d++) out[d] = (g[d] - n[d] * dot) / len;
    }
    g_sum[3 * v] = out[0]; g_sum[3 * v + 1] = out[1]; g_sum[3 * v + 2] = out[2];
}

template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_normals_bwd_face(int V, int F, const Idx* __restrict__ faces, const double* __restrict__ g_sum, double* __restrict__ g_face)
{
    const size_t f = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (f >= (size_t)F) return;
    long long i[3];
    double g[3] = {0.0, 0.0, 0.0};
    if (mg_load_face(faces, f, V, i)) {
#pragma unroll
        for (int d = 0; d < 3; d++) g[d] = (g_sum[3 * i[0] + d] + g_sum[3 * i[1] + d]) + g_sum[3 * i[2] + d];
    }
    g_face[3 * f] = g[0]; g_face[3 * f + 1] = g[1]; g_face[3 * f + 2] = g[2];
}

// with e1 = v1 - v0, e2 = v2 - v0 and G the face's gradient: dL/de1 = e2 x G, dL/de2 = G x e1; corner 1 receives the first, corner 2 the
// second, corner 0 minus both.  Plain arithmetic: 0 * NaN stays a NaN, as in the framework's backward.
template <typename Idx>
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_normals_bwd_gather(int V, int F, const float* __restrict__ v_pos, const Idx* __restrict__ faces,
                                                                    const uint32_t* __restrict__ inc_end, const uint32_t* __restrict__ inc, const double* __restrict__ g_face,
                                                                    float* __restrict__ d_pos)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= (size_t)V) return;
    double acc[3] = {0.0, 0.0, 0.0};
    const Run run = run_bounds(inc_end, v, 3 * (size_t)F);
    for (size_t k = run.lo; k < run.hi; k++) {
        const uint32_t x = inc[k];
        const size_t f = x / 3u;
        const int c = (int)(x - 3u * (uint32_t)f);
        long long i[3];
        if (f >= (size_t)F || !mg_load_face(faces, f, V, i) || i[c] != (long long)v) continue;
        double p0[3], p1[3], p2[3], e1[3], e2[3], G[3], t1[3], t2[3];
        mg_row(v_pos, i[0], p0); mg_row(v_pos, i[1], p1); mg_row(v_pos, i[2], p2);
#pragma unroll
        for (int d = 0; d < 3; d++) { e1[d] = p1[d] - p0[d]; e2[d] = p2[d] - p0[d]; G[d] = g_face[3 * f + d]; }
        mg_cross(e2, G, t1);
        mg_cross(G, e1, t2);
#pragma unroll
        for (int d = 0; d < 3; d++) acc[d] += c == 0 ? -t1[d] - t2[d] : c == 1 ? t1[d] : t2[d];
    }
    d_pos[3 * v] = (float)acc[0]; d_pos[3 * v + 1] = (float)acc[1]; d_pos[3 * v + 2] = (float)acc[2];
}

// ---- the two losses: per-workgroup sums in double, then one workgroup over the partial sums ----
__device__ __forceinline__ double mg_block_sum(double x, double* lds)       // a fixed tree: the same bits every run; valid in thread 0
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < RUN_BLOCK / 64; k++) s += lds[k];
    }
    __syncthreads();
    return s;
}
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_mean(size_t n_partial, const double* __restrict__ partial, double count, float* __restrict__ out)
{
    __shared__ double lds[4];
    double s = 0.0;
    for (size_t k = threadIdx.x; k < n_partial; k += RUN_BLOCK) s += partial[k];
    s = mg_block_sum(s, lds);
    if (threadIdx.x == 0) *out = (float)(s / count);
}

// cosine similarity as torch evaluates it: each row divided by max(|row|, eps), then the dot product
__device__ __forceinline__ double mg_cosine(const double x[3], const double y[3], double& nx, double& cx, double yh[3])
{
    nx = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    const double ny = sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
    cx = nx > MG_COSINE_EPS ? nx : MG_COSINE_EPS;
    const double cy = ny > MG_COSINE_EPS ? ny : MG_COSINE_EPS;
    yh[0] = y[0] / cy; yh[1] = y[1] / cy; yh[2] = y[2] / cy;
    return (x[0] / cx) * yh[0] + (x[1] / cx) * yh[1] + (x[2] / cx) * yh[2];
}

__global__ __launch_bounds__(RUN_BLOCK) void k_mg_consistency(int V, long long E, const float* __restrict__ v_nrm, const long long* __restrict__ edges, double* __restrict__ partial)
{
    __shared__ double lds[4];
    const long long e = (long long)blockIdx.x * RUN_BLOCK + threadIdx.x;
    double term = 0.0;
    if (e < E) {
        const long long a = edges[2 * e], b = edges[2 * e + 1];
        if ((unsigned long long)a < (unsigned long long)V && (unsigned long long)b < (unsigned long long)V) {
            double x[3], y[3], yh[3], nx, cx;
            mg_row(v_nrm, a, x); mg_row(v_nrm, b, y);
            term = 1.0 - mg_cosine(x, y, nx, cx, yh);
        }
    }
    term = mg_block_sum(term, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = term;
}

// d cos / d x for the pair (x, y): (y^ - cos [|x| >= eps] x / |x|) / max(|x|, eps)
__device__ __forceinline__ void mg_cosine_grad(const float* __restrict__ v_nrm, const double x[3], long long other, double acc[3])
{
    double y[3], yh[3], nx, cx;
    mg_row(v_nrm, other, y);
    const double c = mg_cosine(x, y, nx, cx, yh);
    const bool live = nx >= MG_COSINE_EPS;
#pragma unroll
    for (int d = 0; d < 3; d++) acc[d] += (yh[d] - (live ? c * (x[d] / nx) : 0.0)) / cx;
}
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_consistency_bwd(int V, long long E, const float* __restrict__ v_nrm, const long long* __restrict__ edges,
                                                                 const uint32_t* __restrict__ edge_end, const uint32_t* __restrict__ max_end, const uint32_t* __restrict__ max_list,
                                                                 const float* __restrict__ g_out, float* __restrict__ d_nrm)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= (size_t)V) return;
    double x[3], acc[3] = {0.0, 0.0, 0.0};
    mg_row(v_nrm, (long long)v, x);
    Run run = run_bounds(edge_end, v, (size_t)E);
    for (size_t e = run.lo; e < run.hi; e++) {                            // v is the min end
        const long long b = edges[2 * e + 1];
        if (edges[2 * e] == (long long)v && (unsigned long long)b < (unsigned long long)V) mg_cosine_grad(v_nrm, x, b, acc);
    }
    run = run_bounds(max_end, v, (size_t)E);
    for (size_t k = run.lo; k < run.hi; k++) {                            // v is the max end, ascending edge number
        const size_t e = max_list[k];
        if (e >= (size_t)E) continue;
        const long long a = edges[2 * e];
        if (edges[2 * e + 1] == (long long)v && (unsigned long long)a < (unsigned long long)V) mg_cosine_grad(v_nrm, x, a, acc);
    }
    const double w = -(double)*g_out / (double)E;
    d_nrm[3 * v] = (float)(w * acc[0]); d_nrm[3 * v + 1] = (float)(w * acc[1]); d_nrm[3 * v + 2] = (float)(w * acc[2]);
}

// sum over v's distinct neighbours o != v of (x[v] - x[o]): the min-end run, then the max-end list.  A pair (v, v) adds -1 and +1 to the
// diagonal in the reference's sparse construction: nothing.
template <typename T>
__device__ __forceinline__ void mg_laplace_row(int V, long long E, const T* __restrict__ x, const long long* __restrict__ edges, const uint32_t* __restrict__ edge_end,
                                               const uint32_t* __restrict__ max_end, const uint32_t* __restrict__ max_list, size_t v, double r[3])
{
    const double x0 = x[3 * v], x1 = x[3 * v + 1], x2 = x[3 * v + 2];
    r[0] = r[1] = r[2] = 0.0;
    Run run = run_bounds(edge_end, v, (size_t)E);
    for (size_t e = run.lo; e < run.hi; e++) {
        const long long o = edges[2 * e + 1];
        if (edges[2 * e] != (long long)v || o == (long long)v || (unsigned long long)o >= (unsigned long long)V) continue;
        r[0] += x0 - (double)x[3 * o]; r[1] += x1 - (double)x[3 * o + 1]; r[2] += x2 - (double)x[3 * o + 2];
    }
    run = run_bounds(max_end, v, (size_t)E);
    for (size_t k = run.lo; k < run.hi; k++) {
        const size_t e = max_list[k];
        if (e >= (size_t)E) continue;
        const long long o = edges[2 * e];
        if (edges[2 * e + 1] != (long long)v || o == (long long)v || (unsigned long long)o >= (unsigned long long)V) continue;
        r[0] += x0 - (double)x[3 * o]; r[1] += x1 - (double)x[3 * o + 1]; r[2] += x2 - (double)x[3 * o + 2];
    }
}
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_laplacian(int V, long long E, const float* __restrict__ v_pos, const long long* __restrict__ edges,
                                                           const uint32_t* __restrict__ edge_end, const uint32_t* __restrict__ max_end, const uint32_t* __restrict__ max_list,
                                                           double* __restrict__ unit_rows, double* __restrict__ partial)
{
    __shared__ double lds[4];
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    double norm = 0.0;
    if (v < (size_t)V) {
        double r[3];
        mg_laplace_row(V, E, v_pos, edges, edge_end, max_end, max_list, v, r);
        norm = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (unit_rows) {                                                 // the norm's gradient: a zero row gets the zero subgradient
            const bool zero = norm == 0.0;
            unit_rows[3 * v] = zero ? 0.0 : r[0] / norm; unit_rows[3 * v + 1] = zero ? 0.0 : r[1] / norm; unit_rows[3 * v + 2] = zero ? 0.0 : r[2] / norm;
        }
    }
    norm = mg_block_sum(norm, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = norm;
}
__global__ __launch_bounds__(RUN_BLOCK) void k_mg_laplacian_bwd(int V, long long E, const long long* __restrict__ edges, const uint32_t* __restrict__ edge_end,
                                                               const uint32_t* __restrict__ max_end, const uint32_t* __restrict__ max_list, const double* __restrict__ unit_rows,
                                                               const float* __restrict__ g_out, float* __restrict__ d_pos)
{
    const size_t v = (size_t)blockIdx.x * RUN_BLOCK + threadIdx.x;
    if (v >= (size_t)V) return;
    double r[3];
    mg_laplace_row(V, E, unit_rows, edges, edge_end, max_end, max_list, v, r);     // the operator is symmetric
    const double w = (double)*g_out / (double)V;
    d_pos[3 * v] = (float)(w * r[0]); d_pos[3 * v + 1] = (float)(w * r[1]); d_pos[3 * v + 2] = (float)(w * r[2]);
}

static inline bool mg_sizes_ok(int V, int F) { return V >= 0 && F >= 0 && (long long)F <= MG_MAX_FACES; }
static inline bool mg_flag_ok(int is64) { return is64 == 0 || is64 == 1; }

}  // namespace tgs

extern "C" {
#include "../../include/tgs_raster.h"

size_t tgs_meshgeom_workspace_bytes(int V, int F)
{
    tgs::MgWork w;
    if (!tgs::mg_sizes_ok(V, F)) return 0;
    return tgs::mg_carve(w, nullptr, (size_t)V, (size_t)F);
}

size_t tgs_meshgeom_table_bytes(int F)
{
    if (!tgs::mg_sizes_ok(0, F)) return 0;
    return tgs::mg_table_capacity((size_t)F) * sizeof(unsigned long long) + 256;
}

size_t tgs_meshgeom_normals_backward_workspace_bytes(int V, int F)
{
    tgs::MgGradWork w;
    if (!tgs::mg_sizes_ok(V, F)) return 0;
    return tgs::mg_grad_carve(w, nullptr, (size_t)V, (size_t)F);
}

int tgs_meshgeom_topology_count(void* stream, int V, int F, const void* faces, int faces_is_int64, uint32_t* inc_end, uint32_t* edge_end, uint32_t* max_end,
                                 int64_t* counts, void* table, size_t table_bytes, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (!mg_sizes_ok(V, F) || F == 0 || !faces || !mg_flag_ok(faces_is_int64) || !inc_end || !counts || !workspace || (table && (!edge_end || !max_end)))
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_topology_count: V >= 0, 0 < F <= (2^32 - 1) / 3, faces_is_int64 in {0, 1}, non-NULL faces / inc_end / counts / workspace, "
                                          "and edge_end / max_end where a table is given, required");
    MgWork w;
    if (mg_carve(w, (char*)workspace, (size_t)V, (size_t)F) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_topology_count: workspace smaller than tgs_meshgeom_workspace_bytes(V, F)");
    const size_t cap = mg_table_capacity((size_t)F);
    if (table && cap * sizeof(unsigned long long) + 256 > table_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_topology_count: table smaller than tgs_meshgeom_table_bytes(F)");
    unsigned long long* keys = table ? (unsigned long long*)(((uintptr_t)table + 255) & ~(uintptr_t)255) : nullptr;
    const size_t row = ((size_t)V + 1) * sizeof(uint32_t);
    if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st) != hipSuccess || hipMemsetAsync(inc_end, 0, row, st) != hipSuccess ||
        (keys && (hipMemsetAsync(keys, 0xff, cap * sizeof(unsigned long long), st) != hipSuccess || hipMemsetAsync(edge_end, 0, row, st) != hipSuccess ||
                  hipMemsetAsync(max_end, 0, row, st) != hipSuccess)))
        return hip_status("tgs_meshgeom_topology_count");
    long long* cnt = (long long*)counts;
    if (faces_is_int64) hipLaunchKernelGGL(k_mg_count<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, V, F, (const long long*)faces, inc_end, edge_end, max_end, cap, keys, cnt);
    else                hipLaunchKernelGGL(k_mg_count<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, V, F, (const int*)faces, inc_end, edge_end, max_end, cap, keys, cnt);
    run_scan(st, inc_end, (size_t)V + 1, w.scan, cnt + 2);
    if (keys) {
        run_scan(st, edge_end, (size_t)V + 1, w.scan, cnt + 0);
        run_scan(st, max_end, (size_t)V + 1, w.scan, (long long*)nullptr);
    }
    return hip_status("tgs_meshgeom_topology_count");
}

int tgs_meshgeom_topology_fill(void* stream, int V, int F, const void* faces, int faces_is_int64, int64_t E, uint32_t* inc_end, uint32_t* inc, uint32_t* edge_end,
                                uint32_t* max_end, int64_t* edges, uint32_t* max_list, const void* table, size_t table_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (!mg_sizes_ok(V, F) || V == 0 || F == 0 || !faces || !mg_flag_ok(faces_is_int64) || !inc_end || !inc || E < 0 || E > 3 * (long long)F ||
        (table && (E == 0 || !edge_end || !max_end || !edges || !max_list)) || (!table && E != 0))
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_topology_fill: V > 0, 0 < F <= (2^32 - 1) / 3, faces_is_int64 in {0, 1}, non-NULL faces / inc_end / inc, and with a table "
                                          "0 < E <= 3 F as tgs_meshgeom_topology_count counted it and non-NULL edge_end / max_end / edges / max_list (without one E = 0) required");
    const size_t cap = mg_table_capacity((size_t)F);
    if (table && cap * sizeof(unsigned long long) + 256 > table_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_topology_fill: table smaller than tgs_meshgeom_table_bytes(F)");
    if (faces_is_int64) hipLaunchKernelGGL(k_mg_inc_fill<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, V, F, (const long long*)faces, inc_end, inc);
    else                hipLaunchKernelGGL(k_mg_inc_fill<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, V, F, (const int*)faces, inc_end, inc);
    hipLaunchKernelGGL(k_mg_sort_u32, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, 3 * (size_t)F, (const uint32_t*)inc_end, inc);
    if (table) {
        const unsigned long long* keys = (const unsigned long long*)(((uintptr_t)table + 255) & ~(uintptr_t)255);
        long long* ed = (long long*)edges;
        hipLaunchKernelGGL(k_edge_fill, run_grid(cap), dim3(RUN_BLOCK), 0, st, V, (long long)E, cap, keys, edge_end, ed);
        hipLaunchKernelGGL(k_edge_sort, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, (long long)E, (const uint32_t*)edge_end, ed);
        hipLaunchKernelGGL(k_mg_max_fill, run_grid((size_t)E), dim3(RUN_BLOCK), 0, st, V, (long long)E, (const long long*)ed, max_end, max_list);
        hipLaunchKernelGGL(k_mg_sort_u32, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, (size_t)E, (const uint32_t*)max_end, max_list);
    }
    return hip_status("tgs_meshgeom_topology_fill");
}

int tgs_meshgeom_normals(void* stream, int V, int F, const float* v_pos, const void* faces, int faces_is_int64, const uint32_t* inc_end, const uint32_t* inc, float* v_nrm)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (!mg_sizes_ok(V, F) || !mg_flag_ok(faces_is_int64) || (V > 0 && (!v_pos || !v_nrm || !inc_end)) || (V > 0 && F > 0 && (!faces || !inc)))
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_normals: V >= 0, 0 <= F <= (2^32 - 1) / 3, faces_is_int64 in {0, 1} and non-NULL v_pos / faces / inc_end / inc / v_nrm required");
    if (V == 0) return TGS_OK;
    if (faces_is_int64) hipLaunchKernelGGL(k_mg_normals<long long>, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, F, v_pos, (const long long*)faces, inc_end, inc, v_nrm);
    else                hipLaunchKernelGGL(k_mg_normals<int>, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, F, v_pos, (const int*)faces, inc_end, inc, v_nrm);
    return hip_status("tgs_meshgeom_normals");
}

int tgs_meshgeom_normals_backward(void* stream, int V, int F, const float* v_pos, const void* faces, int faces_is_int64, const uint32_t* inc_end, const uint32_t* inc,
                                   const float* dL_dnrm, float* dL_dpos, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (!mg_sizes_ok(V, F) || !mg_flag_ok(faces_is_int64) || !workspace || (V > 0 && (!v_pos || !dL_dnrm || !inc_end)) || (V > 0 && F > 0 && (!faces || !inc)))
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_normals_backward: V >= 0, 0 <= F <= (2^32 - 1) / 3, faces_is_int64 in {0, 1} and non-NULL v_pos / faces / inc_end / inc / "
                                          "dL_dnrm / workspace required");
    MgGradWork w;
    if (mg_grad_carve(w, (char*)workspace, (size_t)V, (size_t)F) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_normals_backward: workspace smaller than tgs_meshgeom_normals_backward_workspace_bytes(V, F)");
    if (!dL_dpos || V == 0) return TGS_OK;
    if (F == 0) {                                                       // nothing reaches a row: zeros
        if (hipMemsetAsync(dL_dpos, 0, 3 * (size_t)V * sizeof(float), st) != hipSuccess) return hip_status("tgs_meshgeom_normals_backward");
        return TGS_OK;
    }
    if (faces_is_int64) {
        const long long* fc = (const long long*)faces;
        hipLaunchKernelGGL(k_mg_normals_bwd_vertex<long long>, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, F, v_pos, fc, inc_end, inc, dL_dnrm, w.g_sum);
        hipLaunchKernelGGL(k_mg_normals_bwd_face<long long>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, V, F, fc, (const double*)w.g_sum, w.g_face);
        hipLaunchKernelGGL(k_mg_normals_bwd_gather<long long>, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, F, v_pos, fc, inc_end, inc, (const double*)w.g_face, dL_dpos);
    } else {
        const int* fc = (const int*)faces;
        hipLaunchKernelGGL(k_mg_normals_bwd_vertex<int>, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, F, v_pos, fc, inc_end, inc, dL_dnrm, w.g_sum);
        hipLaunchKernelGGL(k_mg_normals_bwd_face<int>, run_grid((size_t)F), dim3(RUN_BLOCK), 0, st, V, F, fc, (const double*)w.g_sum, w.g_face);
        hipLaunchKernelGGL(k_mg_normals_bwd_gather<int>, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, F, v_pos, fc, inc_end, inc, (const double*)w.g_face, dL_dpos);
    }
    return hip_status("tgs_meshgeom_normals_backward");
}

int tgs_meshgeom_consistency(void* stream, int V, int64_t E, const float* v_nrm, const int64_t* edges, float* out, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V <= 0 || E <= 0 || E > 3 * MG_MAX_FACES || !v_nrm || !edges || !out || !workspace)
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_consistency: V > 0, 0 < E < 2^32 and non-NULL v_nrm / edges / out / workspace required");
    MgWork w;
    if (mg_carve(w, (char*)workspace, (size_t)V, (size_t)((E + 2) / 3)) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_consistency: workspace smaller than tgs_meshgeom_workspace_bytes(V, ceil(E / 3))");
    hipLaunchKernelGGL(k_mg_consistency, run_grid((size_t)E), dim3(RUN_BLOCK), 0, st, V, (long long)E, v_nrm, (const long long*)edges, w.partial);
    hipLaunchKernelGGL(k_mg_mean, dim3(1), dim3(RUN_BLOCK), 0, st, run_blocks((size_t)E), (const double*)w.partial, (double)E, out);
    return hip_status("tgs_meshgeom_consistency");
}

int tgs_meshgeom_consistency_backward(void* stream, int V, int64_t E, const float* v_nrm, const int64_t* edges, const uint32_t* edge_end, const uint32_t* max_end,
                                       const uint32_t* max_list, const float* dL_dout, float* dL_dnrm)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V <= 0 || E <= 0 || E > 3 * MG_MAX_FACES || !v_nrm || !edges || !edge_end || !max_end || !max_list || !dL_dout)
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_consistency_backward: V > 0, 0 < E < 2^32 and non-NULL v_nrm / edges / edge_end / max_end / max_list / dL_dout required");
    if (!dL_dnrm) return TGS_OK;
    hipLaunchKernelGGL(k_mg_consistency_bwd, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, (long long)E, v_nrm, (const long long*)edges, edge_end, max_end, max_list, dL_dout, dL_dnrm);
    return hip_status("tgs_meshgeom_consistency_backward");
}

int tgs_meshgeom_laplacian(void* stream, int V, int64_t E, const float* v_pos, const int64_t* edges, const uint32_t* edge_end, const uint32_t* max_end,
                            const uint32_t* max_list, double* unit_rows, float* out, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V <= 0 || E < 0 || E > 3 * MG_MAX_FACES || !v_pos || !edge_end || !max_end || !out || !workspace || (E > 0 && (!edges || !max_list)))
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_laplacian: V > 0, 0 <= E < 2^32 and non-NULL v_pos / edges / edge_end / max_end / max_list / out / workspace required");
    MgWork w;
    if (mg_carve(w, (char*)workspace, (size_t)V, (size_t)((E + 2) / 3)) > workspace_bytes)
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_laplacian: workspace smaller than tgs_meshgeom_workspace_bytes(V, ceil(E / 3))");
    hipLaunchKernelGGL(k_mg_laplacian, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, (long long)E, v_pos, (const long long*)edges, edge_end, max_end, max_list, unit_rows, w.partial);
    hipLaunchKernelGGL(k_mg_mean, dim3(1), dim3(RUN_BLOCK), 0, st, run_blocks((size_t)V), (const double*)w.partial, (double)V, out);
    return hip_status("tgs_meshgeom_laplacian");
}

int tgs_meshgeom_laplacian_backward(void* stream, int V, int64_t E, const int64_t* edges, const uint32_t* edge_end, const uint32_t* max_end, const uint32_t* max_list,
                                     const double* unit_rows, const float* dL_dout, float* dL_dpos)
{
    using namespace tgs;
    hipStream_t st = (hipStream_t)stream;
    if (V <= 0 || E < 0 || E > 3 * MG_MAX_FACES || !edge_end || !max_end || !unit_rows || !dL_dout || (E > 0 && (!edges || !max_list)))
        return set_error(TGS_ERR_INVALID, "tgs_meshgeom_laplacian_backward: V > 0, 0 <= E < 2^32 and non-NULL edges / edge_end / max_end / max_list / unit_rows / dL_dout required");
    if (!dL_dpos) return TGS_OK;
    hipLaunchKernelGGL(k_mg_laplacian_bwd, run_grid((size_t)V), dim3(RUN_BLOCK), 0, st, V, (long long)E, (const long long*)edges, edge_end, max_end, max_list, unit_rows, dL_dout, dL_dpos);
    return hip_status("tgs_meshgeom_laplacian_backward");
}
}
