// tgs_depth.hip -- expected depth of a finished colour frame and its gradients, for gfx950 (wave64).
//
//   k_depth_fwd        depth(p) = sum_i T_i(p) alpha_i(p) z_i over exactly the (pixel, entry) pairs the colour frame blended
//   k_depth_bwd        back to front: the gradient of that sum through alpha_i (added into the slab rows the colour's per-pixel backward
//                      has written) and through z_i (a per-instance scratch row)
//   k_depth_bwd_gauss  per Gaussian: sum of its dz rows, times the third row of the view transform, added to dL_dmeans3D
//   k_depth_bwd_gauss_views  the same for every view of a batch in one pass (tgs_backward_batch_depth_range)
//
// A pass of its own over the state every frame already stores (sorted records, n_contrib, final_T, the sorted keys): the render pair is not
// touched and nothing here runs unless depth is asked for.  Geometry as k_render_bwd_det: 256 threads per tile, one lane per pixel, wave w
// owns the 8x8-pixel quadrant w and walks only the staged entries whose block mask reaches it.  Which pairs were blended is replayed, not
// stored: positions 1 .. n_contrib[pixel] that pass the two cut-offs (power > 0, alpha < 1/255), with alpha from the instruction sequence of
// the render kernels (pair_power2 on the conic scaled as stage_conic_* scales it, v_exp_f32) -- so every pair falls on the side of 1/255 it
// fell on in the colour frame (the plain-function pieces of this are shared: tgs_replay.hpp).  No termination test: n_contrib is the position of the last BLENDED entry.
// z_i is the high word of the instance's sorted key (k_scatter: bits(GeomState::depth) << 32 | index), which lies beside the records.
// No float atomics: per-wave sums in DPP, waves in a fixed order through LDS, one writer per row -- two runs give the same bits.
#include "tgs_replay.hpp"

namespace tgs {

constexpr int DACC = 7;        // mean2D xy, conic xx / xy / yy, opacity, z (of wave_reduce36's RCOMP components the two spare ones stay zero)

// ---------------------------------------------------------------------------------------------
// k_depth_fwd: one workgroup per tile of tile_desc (workgroups behind the tiles with instances return: the output is zero-filled in front
// of the launch, which is also what a rejected frame and a tile without instances keep).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_depth_fwd(const ImgState s, const BinState b, int W, int H, uint32_t gx, float* __restrict__ out_depth)
{
    __shared__ float4 sA[RCHUNK + 1];
    __shared__ float4 sB[RCHUNK + 1];
    __shared__ float sZ[RCHUNK + 1];
    __shared__ QuadLists L;
    __shared__ uint32_t wmax[4];

    const uint2 ff = frame_flags(s);
    if ((ff.x & META_ERR_CAPACITY) || blockIdx.x >= ff.y) return;
    const ReplayLane ln = replay_lane(s, gx, W, H);
    const int wv = ln.wv, lane = ln.lane;
    const uint32_t start = ln.start, n = ln.n;
    const uint32_t last_contributor = ln.inside ? s.n_contrib[ln.pix_id] : 0u;
    const uint32_t qmax = min(tile_deepest(last_contributor, wmax, wv, lane), n);
    if (qmax == 0) return;
    if (threadIdx.x == 0) { sA[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f); sB[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f); sZ[RNULL] = 0.f; }

    float T = 1.0f, D = 0.f;
    for (uint32_t base = 0; base < qmax; base += RCHUNK) {
        const uint32_t cnt = min((uint32_t)RCHUNK, qmax - base);
        __syncthreads();                                    // the previous round's records have been read
        uint32_t qm = 0;
        if (threadIdx.x < cnt) {
            const uint32_t pos = start + base + threadIdx.x;
            sA[threadIdx.x] = b.recA[pos]; sB[threadIdx.x] = b.recB[pos];
            sZ[threadIdx.x] = __uint_as_float((uint32_t)(b.keys[pos] >> 32));
            qm = block_to_quadrant_mask(__float_as_uint(b.recC[pos].y));
        }
        build_quad_lists(L, qm, wv, lane);
        __syncthreads();
#pragma unroll 1
        for (int sw = 0; sw < 4; sw++) {                    // staging waves in order: the quadrant's entries front to back
            const uint32_t nl = __builtin_amdgcn_readfirstlane(L.cnt[wv][sw]);
#pragma unroll 1
            for (uint32_t k = 0; k < nl; k += RUNROLL) {
                const uint2 pk = *reinterpret_cast<const uint2*>(&L.idx[wv][sw][k]);
                const uint32_t j[RUNROLL] = {pk.x & 0xffffu, pk.x >> 16, pk.y & 0xffffu, pk.y >> 16};
                float4 a[RUNROLL], bb[RUNROLL];
                float z[RUNROLL];
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) { a[u] = sA[j[u]]; bb[u] = sB[j[u]]; z[u] = sZ[j[u]]; }
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) {
                    float G; bool cut;
                    const float alpha = replay_pair_alpha(a[u], bb[u], a[u].x - ln.pixfx, a[u].y - ln.pixfy, G, cut);
                    // 1-based list position base + j + 1 <= n_contrib; a padding entry (slot RNULL) has opacity 0 and is cut
                    if (base + j[u] < last_contributor && !cut) {
                        D += z[u] * (alpha * T);
                        T = T * (1.f - alpha);
                    }
                }
            }
        }
    }
    if (ln.inside) out_depth[ln.pix_id] = D;
}

// ---------------------------------------------------------------------------------------------
// k_depth_bwd: backward.cu:486-541 with z where the colour stands, one channel, no background term.  Per blended pair, back to front:
//   T <- T / (1 - alpha)  (from final_T),   dz += g alpha T,   dL_dalpha = g T (z - accum_rec),   accum_rec <- alpha z + (1 - alpha) accum_rec
// and from dL_dalpha the mean2D, conic and opacity terms as the colour's (backward.cu:537-555).  Entry j's sums over the tile's pixels:
// wave_reduce36 inside a wave, the four waves in order at the flush, which ADDS them into the instance's slab row (written by k_render_bwd*
// in front of this kernel on the same stream; a row has one writer: this tile's workgroup) and stores dz to dz_rows[slot].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_depth_bwd(const ImgState s, const BinState b, int W, int H, uint32_t gx, const float* __restrict__ dL_ddepth,
                                                   float* __restrict__ dz_rows)
{
    __shared__ float4 sA[RCHUNK + 1];
    __shared__ float4 sB[RCHUNK + 1];
    __shared__ float sZ[RCHUNK + 1];
    __shared__ uint32_t sSlot[RCHUNK];
    __shared__ float wacc[4][DACC][RCHUNK + 1];            // per-wave partial sums of the current round (+1: null slot)
    __shared__ unsigned long long touched[4][RCHUNK / 64];
    __shared__ QuadLists L;
    __shared__ uint32_t wmax[4];

    const uint2 ff = frame_flags(s);
    if ((ff.x & META_ERR_CAPACITY) || blockIdx.x >= ff.y) return;
    const ReplayLane ln = replay_lane(s, gx, W, H);
    const int wv = ln.wv, lane = ln.lane;
    const uint32_t start = ln.start, n = ln.n;
    float T = ln.inside ? s.final_T[ln.pix_id] : 0.f;
    const uint32_t last_contributor = ln.inside ? s.n_contrib[ln.pix_id] : 0u;
    const float g = ln.inside ? dL_ddepth[ln.pix_id] : 0.f;
    const uint32_t qmax = min(tile_deepest(last_contributor, wmax, wv, lane), n);
    if (qmax == 0) return;                                  // (dz_rows is zero-filled in front of the launch: rows behind qmax keep 0)
    if (threadIdx.x == 0) { sA[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f); sB[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f); sZ[RNULL] = 0.f; }
    float acc = 0.f, last_alpha = 0.f, last_z = 0.f;        // accum_rec and the entry behind it
    const float ddelx_dx = (float)(0.5 * W), ddely_dy = (float)(0.5 * H);   // backward.cu:460-461

    // slot t of a round = list position qhi - 1 - t: back to front
    for (uint32_t qhi = qmax; qhi > 0; qhi = qhi > RCHUNK ? qhi - RCHUNK : 0) {
        const uint32_t cnt = min((uint32_t)RCHUNK, qhi);
        __syncthreads();                                    // the previous round's flush has read wacc / sSlot
        uint32_t qm = 0;
        if (threadIdx.x < cnt) {
            const uint32_t pos = start + qhi - 1 - threadIdx.x;
            sA[threadIdx.x] = b.recA[pos]; sB[threadIdx.x] = b.recB[pos];
            sZ[threadIdx.x] = __uint_as_float((uint32_t)(b.keys[pos] >> 32));
            sSlot[threadIdx.x] = b.slot[pos];
            qm = block_to_quadrant_mask(__float_as_uint(b.recC[pos].y));
        }
        build_quad_lists(L, qm, wv, lane);
        if (lane < RCHUNK / 64) touched[wv][lane] = 0ull;
        __syncthreads();

#pragma unroll 1
        for (int sw = 0; sw < 4; sw++) {
            const uint32_t nl = __builtin_amdgcn_readfirstlane(L.cnt[wv][sw]);
            unsigned long long tmask = 0;
#pragma unroll 1
            for (uint32_t k = 0; k < nl; k += RUNROLL) {
                const uint2 pk = *reinterpret_cast<const uint2*>(&L.idx[wv][sw][k]);
                const uint32_t j[RUNROLL] = {pk.x & 0xffffu, pk.x >> 16, pk.y & 0xffffu, pk.y >> 16};
                float4 a[RUNROLL], bb[RUNROLL];
                float z[RUNROLL], dx[RUNROLL], dy[RUNROLL], G[RUNROLL], alpha[RUNROLL];
                bool valid[RUNROLL];
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) { a[u] = sA[j[u]]; bb[u] = sB[j[u]]; z[u] = sZ[j[u]]; }
                bool any = false;
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) {
                    dx[u] = a[u].x - ln.pixfx; dy[u] = a[u].y - ln.pixfy;
                    bool cut;
                    alpha[u] = replay_pair_alpha(a[u], bb[u], dx[u], dy[u], G[u], cut);
                    valid[u] = (qhi - 1 - j[u] < last_contributor) && (j[u] < cnt) && !cut;
                    any = any || valid[u];
                }
                if (__builtin_amdgcn_ballot_w64(any) == 0) continue;
                float v[RUNROLL * RCOMP];
#pragma unroll
                for (int i = 0; i < RUNROLL * RCOMP; i++) v[i] = 0.f;
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) {
                    if (valid[u]) {
                        const float om = 1.f - alpha[u];
                        T = tgs_div(T, om);
                        acc = last_alpha * last_z + (1.f - last_alpha) * acc;
                        last_z = z[u]; last_alpha = alpha[u];
                        const float dL_dalpha = (z[u] - acc) * g * T;
                        geometry_terms<RCOMP, 0>(v, u, a[u], bb[u], dx[u], dy[u], G[u], dL_dalpha, ddelx_dx, ddely_dy);
                        v[u * RCOMP + 6] = g * (alpha[u] * T);
                    }
                }
                float r[RCOMP];
                wave_reduce36(v, r);                        // row e of r[k]: total of entry e, component k
                const int row = lane >> 4;
                const uint32_t jr = row == 0 ? j[0] : row == 1 ? j[1] : row == 2 ? j[2] : j[3];
                if ((lane & 15) == 0) {                     // (null slots go to the spare column)
#pragma unroll
                    for (int c = 0; c < DACC; c++) wacc[wv][c][jr] = r[c];
                }
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) if (j[u] < RCHUNK) tmask |= 1ull << (j[u] & 63);
            }
            if (lane == 0 && tmask) touched[wv][sw] = tmask;
        }
        __syncthreads();
        // flush: thread j adds the (up to) 4 wave partials of entry j in wave order, then its slab row <- row + sums
        if (threadIdx.x < cnt) {
            const uint32_t j = threadIdx.x;
            float r[DACC];
            double rc[3] = {0.0, 0.0, 0.0};
            bool some = false;
#pragma unroll
            for (int k = 0; k < DACC; k++) r[k] = 0.f;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                if ((touched[w][j >> 6] >> (j & 63)) & 1ull) {
                    some = true;
#pragma unroll
                    for (int k = 0; k < DACC; k++) r[k] += wacc[w][k][j];
#pragma unroll
                    for (int k = 0; k < 3; k++) rc[k] += (double)wacc[w][2 + k][j];
                }
            }
            if (some) {
                const uint32_t slot = sSlot[j];
                slab_row_add(b.slab + (size_t)slot * SLAB_ROW, r, rc);
                dz_rows[slot] = r[6];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_depth_bwd_gauss: one lane per Gaussian, behind the per-Gaussian pass (which has written or accumulated dL_dmeans3D):
// dL_dmeans3D += (sum of the Gaussian's dz rows, in row order) * (m[2], m[6], m[10]) -- z = m[2] x + m[6] y + m[10] z + m[14].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PRE_BLOCK) void k_depth_bwd_gauss(int P, const Meta* __restrict__ meta, const int* __restrict__ radii, const GeomState g,
                                                               const float* __restrict__ view, const float* __restrict__ dz_rows, float* __restrict__ dL_dmean3D)
{
    const int idx = blockIdx.x * PRE_BLOCK + threadIdx.x;
    if (idx >= P) return;
    if (__builtin_nontemporal_load(&meta->error) & META_ERR_CAPACITY) return;      // a rejected frame contributes nothing
    if (!(radii[idx] > 0)) return;
    const uint32_t tiles = g.tiles_touched[idx], off = g.offsets[idx];
    float dz = 0.f;
    for (uint32_t k = 0; k < tiles; k++) dz += dz_rows[off + k];
    if (dz == 0.f) return;
    float* o = dL_dmean3D + 3 * (size_t)idx;
    o[0] += dz * view[2]; o[1] += dz * view[6]; o[2] += dz * view[10];
}

// ---------------------------------------------------------------------------------------------
// k_depth_bwd_gauss_views: k_depth_bwd_gauss for the views of a batch, behind the batch's per-Gaussian pass over the same range.  One lane
// per Gaussian of [block0 * PRE_BLOCK, end); the views of the chunk in ascending index, a view's rows in row order, the products summed in
// registers and ONE read-modify-write of dL_dmeans3D per Gaussian and chunk (the per-view kernel: one launch and one read-modify-write per
// view).  No atomics, a fixed order: two runs give the same bits.
// Load-latency bound, not VALU bound: per view a lane does three dependent steps (radii / tiles_touched / offsets -> the dz rows -> three
// multiply-adds) and almost no arithmetic.  So the first step of EVERY view of the chunk is issued before any row is read -- the independent
// loads of up to 8 views are in flight together instead of 8 round trips one behind the other -- and the kernel asks for no occupancy beyond
// what 256-thread groups give: 24 VGPRs, no scratch, every wave slot of a SIMD usable to hide the row walk.  A view's meta / matrix words are uniform (scalar loads).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PRE_BLOCK) void k_depth_bwd_gauss_views(int end, int block0, const DepthViews dv, float* __restrict__ dL_dmean3D)
{
    const int idx = (block0 + (int)blockIdx.x) * PRE_BLOCK + (int)threadIdx.x;
    if (idx >= end) return;
    uint32_t tiles[BATCH_VIEWS], off[BATCH_VIEWS];
#pragma unroll
    for (int k = 0; k < BATCH_VIEWS; k++) {
        tiles[k] = 0; off[k] = 0;
        if (k < dv.n) {
            const DepthView& w = dv.v[k];
            // a rejected frame contributes nothing (and its offsets may point past its capacity: they are not followed)
            const bool live = !(__builtin_nontemporal_load(&w.meta->error) & META_ERR_CAPACITY) && w.radii[idx] > 0;
            if (live) { tiles[k] = w.tiles_touched[idx]; off[k] = w.offsets[idx]; }
        }
    }
    float ax = 0.f, ay = 0.f, az = 0.f;
    bool any = false;
#pragma unroll
    for (int k = 0; k < BATCH_VIEWS; k++) {
        if (k < dv.n && tiles[k] > 0) {
            const DepthView& w = dv.v[k];
            float dz = 0.f;
            for (uint32_t r = 0; r < tiles[k]; r++) dz += w.dz_rows[off[k] + r];
            ax += dz * w.view[2]; ay += dz * w.view[6]; az += dz * w.view[10];
            any = any || dz != 0.f;
        }
    }
    if (!any) return;
    float* o = dL_dmean3D + 3 * (size_t)idx;
    o[0] += ax; o[1] += ay; o[2] += az;
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------
// out_depth[N] <- 0, then the tiles with instances (at most T workgroups have work)
void launch_depth_fwd(hipStream_t st, const ImgState& s, const BinState& b, int W, int H, uint32_t gx, uint32_t T, float* out_depth)
{
    (void)hipMemsetAsync(out_depth, 0, (size_t)W * H * sizeof(float), st);
    if (T > 0) hipLaunchKernelGGL(k_depth_fwd, dim3(T), dim3(256), 0, st, s, b, W, H, gx, out_depth);
}
// tiles: leading entries of tile_order that can hold instances (launch_render_bwd's).  dz_rows[R] <- 0 first: rows the kernel does not visit read as 0.
void launch_depth_bwd(hipStream_t st, const ImgState& s, const BinState& b, int W, int H, uint32_t gx, uint32_t tiles, size_t R, const float* dL_ddepth, float* dz_rows)
{
    (void)hipMemsetAsync(dz_rows, 0, R * sizeof(float), st);
    if (tiles > 0) hipLaunchKernelGGL(k_depth_bwd, dim3(tiles), dim3(256), 0, st, s, b, W, H, gx, dL_ddepth, dz_rows);
}
void launch_depth_bwd_gauss(hipStream_t st, int P, const Meta* meta, const int* radii, const GeomState& g, const float* view, const float* dz_rows, float* dL_dmean3D)
{
    hipLaunchKernelGGL(k_depth_bwd_gauss, dim3((unsigned)n_blocks((size_t)P)), dim3(PRE_BLOCK), 0, st, P, meta, radii, g, view, dz_rows, dL_dmean3D);
}
// Gaussians [first, first + count) of P (first a multiple of PRE_BLOCK), the views of one chunk
void launch_depth_bwd_gauss_views(hipStream_t st, int first, int count, const DepthViews& dv, float* dL_dmean3D)
{
    if (count <= 0 || dv.n <= 0) return;
    hipLaunchKernelGGL(k_depth_bwd_gauss_views, dim3((unsigned)n_blocks((size_t)count)), dim3(PRE_BLOCK), 0, st, first + count, first / PRE_BLOCK, dv, dL_dmean3D);
}

}  // namespace tgs
