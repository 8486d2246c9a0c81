// tgs_feature.hip -- per-Gaussian feature channels composited over a finished colour frame, and their gradients, for gfx950 (wave64).
//
//   k_feat_fwd        feature_map[c](p) = sum_i T_i(p) alpha_i(p) features[i, c] over exactly the (pixel, entry) pairs the colour frame blended
//   k_feat_bwd        back to front: the gradient of those sums through alpha_i (added into the slab rows the colour's per-pixel backward has
//                     written, as k_depth_bwd adds its share) and through features[i, c] (a per-instance scratch row of C floats)
//   k_feat_bwd_gauss  per Gaussian: sum of its scratch rows, in row order, into dL_dfeatures[i, :]
//   k_feat_bwd_gauss_views  the same for every view of a batch in one pass (tgs_backward_batch_features_range)
//
// tgs_depth.hip is the special case "one channel, the feature is z"; geometry, staging and the pair replay are its (256 threads per tile, one
// lane per pixel, wave w owns the 8x8-pixel quadrant w, replay_lane / replay_pair_alpha / tile_deepest / geometry_terms / slab_row_add of tgs_replay.hpp).  The feature row of a staged entry
// is gathered by the Gaussian index, the low word of the instance's sorted key, and lies in LDS beside the records.
// Channels travel in groups of at most FGROUP = 8 per launch (C = 9 .. 16: two launches each way).  The through-alpha share is linear in the
// channels, so each launch adds its own share to the slab rows: launches on one stream are ordered and a row has one writer.  The kernels are
// compiled for 4 and for 8 channel slots (a group of 1 .. 4 channels takes the narrow one; slots behind the group hold zeros and store nothing).
// Signed values, nothing clamped, no float atomics: two runs give the same bits.
#include "tgs_replay.hpp"

namespace tgs {

constexpr int FGROUP = 8;          // channels per launch: 8 channels x 4 entries are one wave_reduce36 call
constexpr int FGEO = 6;            // mean2D xy, conic xx / xy / yy, opacity
// k_feat_bwd stages FCHUNK entries per round, not RCHUNK: the per-wave partial sums are 4 x (6 + 8) x (FCHUNK + 1) floats = 28.9 KB; at 256
// entries they alone would be 57.6 KB on top of the staging arrays.  (The staging arrays keep RCHUNK + 1 slots: RNULL is the lists' padding.)
constexpr int FCHUNK = 128;

// the feature row of Gaussian `idx`, channels c0 .. c0 + nc - 1, into NC slots (zeros behind the group)
template <int NC>
__device__ __forceinline__ void load_feature_row(const float* __restrict__ features, uint32_t idx, int C, int c0, int nc, float4 (&f)[NC / 4])
{
    const float* row = features + (size_t)idx * C + c0;
    float v[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) v[c] = c < nc ? row[c] : 0.f;
#pragma unroll
    for (int q = 0; q < NC / 4; q++) f[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// ---------------------------------------------------------------------------------------------
// k_feat_fwd: one workgroup per tile of tile_desc (the output is zero-filled in front of the launches, which is what a rejected frame, a tile
// without instances and the workgroups behind the tiles with instances keep).  Each accumulation is one fmaf on w = alpha T, so a channel's
// bits do not depend on its slot, its group or the channels that travel with it.
// ---------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void k_feat_fwd(const ImgState s, const BinState b, int W, int H, uint32_t gx, uint32_t P, int C, int c0, int nc,
                                                  const float* __restrict__ features, float* __restrict__ out)
{
    __shared__ float4 sA[RCHUNK + 1];
    __shared__ float4 sB[RCHUNK + 1];
    __shared__ float4 sF[NC / 4][RCHUNK + 1];
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
    if (threadIdx.x == 0) {
        sA[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f); sB[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < NC / 4; q++) sF[q][RNULL] = make_float4(0.f, 0.f, 0.f, 0.f);
    }

    float T = 1.0f, F[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) F[c] = 0.f;
    for (uint32_t base = 0; base < qmax; base += RCHUNK) {
        const uint32_t cnt = min((uint32_t)RCHUNK, qmax - base);
        __syncthreads();                                    // the previous round's records have been read
        uint32_t qm = 0;
        if (threadIdx.x < cnt) {
            const uint32_t pos = start + base + threadIdx.x;
            sA[threadIdx.x] = b.recA[pos]; sB[threadIdx.x] = b.recB[pos];
            float4 f[NC / 4];
            load_feature_row<NC>(features, min((uint32_t)b.keys[pos], P - 1u), C, c0, nc, f);
#pragma unroll
            for (int q = 0; q < NC / 4; q++) sF[q][threadIdx.x] = f[q];
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
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) { a[u] = sA[j[u]]; bb[u] = sB[j[u]]; }
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) {
                    float G; bool cut;
                    const float alpha = replay_pair_alpha(a[u], bb[u], a[u].x - ln.pixfx, a[u].y - ln.pixfy, G, cut);
                    // 1-based list position base + j + 1 <= n_contrib; a padding entry (slot RNULL) has opacity 0 and is cut
                    if (base + j[u] < last_contributor && !cut) {
                        const float w = alpha * T;
#pragma unroll
                        for (int q = 0; q < NC / 4; q++) {
                            const float4 f = sF[q][j[u]];
                            F[4 * q + 0] = fmaf(f.x, w, F[4 * q + 0]); F[4 * q + 1] = fmaf(f.y, w, F[4 * q + 1]);
                            F[4 * q + 2] = fmaf(f.z, w, F[4 * q + 2]); F[4 * q + 3] = fmaf(f.w, w, F[4 * q + 3]);
                        }
                        T = T * (1.f - alpha);
                    }
                }
            }
        }
    }
    if (ln.inside) {
        const size_t N = (size_t)W * H;
#pragma unroll
        for (int c = 0; c < NC; c++) if (c < nc) out[(size_t)(c0 + c) * N + ln.pix_id] = F[c];
    }
}

// ---------------------------------------------------------------------------------------------
// k_feat_bwd: backward.cu:486-541 with the feature where the colour stands, the group's channels, no background term.  Per blended pair,
// back to front:
//   T <- T / (1 - alpha)  (from final_T),   df_c += g_c alpha T,   dL_dalpha = T sum_c g_c (f_c - accum_rec_c),
//   accum_rec_c <- alpha f_c + (1 - alpha) accum_rec_c
// and from dL_dalpha the mean2D, conic and opacity terms as the colour's (backward.cu:537-555).  Entry j's sums over the tile's pixels:
// wave_reduce36 inside a wave (the six geometry sums are one call, the channels a second), the four waves in order at the flush, which ADDS
// the geometry sums into the instance's slab row (hi + lo for the conic, as k_depth_bwd) and stores the channel sums to
// feat_rows[slot * C + c0 ..] (zero-filled in front of the launches; a row has one writer: this tile's workgroup).
// ---------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void k_feat_bwd(const ImgState s, const BinState b, int W, int H, uint32_t gx, uint32_t P, int C, int c0, int nc,
                                                  const float* __restrict__ features, const float* __restrict__ dL_dmap, float* __restrict__ feat_rows)
{
    constexpr int FACC = FGEO + NC;
    __shared__ float4 sA[RCHUNK + 1];
    __shared__ float4 sB[RCHUNK + 1];
    __shared__ float4 sF[NC / 4][RCHUNK + 1];
    __shared__ uint32_t sSlot[FCHUNK];
    __shared__ float wacc[4][FACC][FCHUNK + 1];            // per-wave partial sums of the current round (+1: null slot)
    __shared__ unsigned long long touched[4][FCHUNK / 64];
    __shared__ QuadLists L;
    __shared__ uint32_t wmax[4];

    const uint2 ff = frame_flags(s);
    if ((ff.x & META_ERR_CAPACITY) || blockIdx.x >= ff.y) return;
    const ReplayLane ln = replay_lane(s, gx, W, H);
    const int wv = ln.wv, lane = ln.lane;
    const uint32_t start = ln.start, n = ln.n;
    float T = ln.inside ? s.final_T[ln.pix_id] : 0.f;
    const uint32_t last_contributor = ln.inside ? s.n_contrib[ln.pix_id] : 0u;
    const uint32_t qmax = min(tile_deepest(last_contributor, wmax, wv, lane), n);
    if (qmax == 0) return;                                  // (feat_rows is zero-filled in front of the launches: rows behind qmax keep 0)
    if (threadIdx.x == 0) {
        sA[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f); sB[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < NC / 4; q++) sF[q][RNULL] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float g[NC], acc[NC], last_f[NC], last_alpha = 0.f;     // upstream, accum_rec and the entry behind it, per channel
    {
        const size_t N = (size_t)W * H;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            g[c] = (ln.inside && c < nc) ? dL_dmap[(size_t)(c0 + c) * N + ln.pix_id] : 0.f;
            acc[c] = 0.f; last_f[c] = 0.f;
        }
    }
    const float ddelx_dx = (float)(0.5 * W), ddely_dy = (float)(0.5 * H);   // backward.cu:460-461

    // slot t of a round = list position qhi - 1 - t: back to front
    for (uint32_t qhi = qmax; qhi > 0; qhi = qhi > FCHUNK ? qhi - FCHUNK : 0) {
        const uint32_t cnt = min((uint32_t)FCHUNK, qhi);
        __syncthreads();                                    // the previous round's flush has read wacc / sSlot
        uint32_t qm = 0;
        if (threadIdx.x < cnt) {
            const uint32_t pos = start + qhi - 1 - threadIdx.x;
            sA[threadIdx.x] = b.recA[pos]; sB[threadIdx.x] = b.recB[pos];
            float4 f[NC / 4];
            load_feature_row<NC>(features, min((uint32_t)b.keys[pos], P - 1u), C, c0, nc, f);
#pragma unroll
            for (int q = 0; q < NC / 4; q++) sF[q][threadIdx.x] = f[q];
            sSlot[threadIdx.x] = b.slot[pos];
            qm = block_to_quadrant_mask(__float_as_uint(b.recC[pos].y));
        }
        build_quad_lists(L, qm, wv, lane);
        if (lane < FCHUNK / 64) touched[wv][lane] = 0ull;
        __syncthreads();

#pragma unroll 1
        for (int sw = 0; sw < FCHUNK / 64; sw++) {          // (the staging waves behind FCHUNK / 64 staged nothing: their lists are empty)
            const uint32_t nl = __builtin_amdgcn_readfirstlane(L.cnt[wv][sw]);
            unsigned long long tmask = 0;
#pragma unroll 1
            for (uint32_t k = 0; k < nl; k += RUNROLL) {
                const uint2 pk = *reinterpret_cast<const uint2*>(&L.idx[wv][sw][k]);
                const uint32_t j[RUNROLL] = {pk.x & 0xffffu, pk.x >> 16, pk.y & 0xffffu, pk.y >> 16};
                float4 a[RUNROLL], bb[RUNROLL];
                float dx[RUNROLL], dy[RUNROLL], G[RUNROLL], alpha[RUNROLL];
                bool valid[RUNROLL];
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) { a[u] = sA[j[u]]; bb[u] = sB[j[u]]; }
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
                float v[RUNROLL * RCOMP], vf[RUNROLL * RCOMP];                        // geometry and channel sums of the 4 entries
#pragma unroll
                for (int i = 0; i < RUNROLL * RCOMP; i++) { v[i] = 0.f; vf[i] = 0.f; }
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) {
                    if (valid[u]) {
                        const float om = 1.f - alpha[u];
                        T = tgs_div(T, om);
                        const float w = alpha[u] * T;
                        float fu[NC];
#pragma unroll
                        for (int q = 0; q < NC / 4; q++) {
                            const float4 f = sF[q][j[u]];
                            fu[4 * q] = f.x; fu[4 * q + 1] = f.y; fu[4 * q + 2] = f.z; fu[4 * q + 3] = f.w;
                        }
                        float sum = 0.f;
#pragma unroll
                        for (int c = 0; c < NC; c++) {
                            acc[c] = last_alpha * last_f[c] + (1.f - last_alpha) * acc[c];
                            last_f[c] = fu[c];
                            sum += (fu[c] - acc[c]) * g[c];
                            vf[u * RCOMP + c] = g[c] * w;
                        }
                        last_alpha = alpha[u];
                        const float dL_dalpha = sum * T;
                        geometry_terms<RCOMP, 0>(v, u, a[u], bb[u], dx[u], dy[u], G[u], dL_dalpha, ddelx_dx, ddely_dy);
                    }
                }
                float r[RCOMP], rf[RCOMP];
                wave_reduce36(v, r);                        // row e of r[k]: total of entry e, component k
                wave_reduce36(vf, rf);
                const int row = lane >> 4;
                const uint32_t je = row == 0 ? j[0] : row == 1 ? j[1] : row == 2 ? j[2] : j[3];
                const uint32_t jr = min(je, (uint32_t)FCHUNK);   // (null slots go to the spare column)
                if ((lane & 15) == 0) {
#pragma unroll
                    for (int c = 0; c < FGEO; c++) wacc[wv][c][jr] = r[c];
#pragma unroll
                    for (int c = 0; c < NC; c++) wacc[wv][FGEO + c][jr] = rf[c];
                }
#pragma unroll
                for (int u = 0; u < RUNROLL; u++) if (j[u] < FCHUNK) tmask |= 1ull << (j[u] & 63);
            }
            if (lane == 0 && tmask) touched[wv][sw] = tmask;
        }
        __syncthreads();
        // flush: thread j adds the (up to) 4 wave partials of entry j in wave order, then its slab row <- row + sums
        if (threadIdx.x < cnt) {
            const uint32_t j = threadIdx.x;
            float r[FACC];
            double rc[3] = {0.0, 0.0, 0.0};
            bool some = false;
#pragma unroll
            for (int k = 0; k < FACC; k++) r[k] = 0.f;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                if ((touched[w][j >> 6] >> (j & 63)) & 1ull) {
                    some = true;
#pragma unroll
                    for (int k = 0; k < FACC; k++) r[k] += wacc[w][k][j];
#pragma unroll
                    for (int k = 0; k < 3; k++) rc[k] += (double)wacc[w][2 + k][j];
                }
            }
            if (some) {
                const uint32_t slot = sSlot[j];
                slab_row_add(b.slab + (size_t)slot * SLAB_ROW, r, rc);
                float* fr = feat_rows + (size_t)slot * C + c0;
#pragma unroll
                for (int c = 0; c < NC; c++) if (c < nc) fr[c] = r[FGEO + c];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_feat_bwd_gauss: one lane per Gaussian: dL_dfeatures[i, c] = (or +=, with `accumulate`) the sum of the Gaussian's scratch rows in row order.
// A culled Gaussian and every Gaussian of a rejected frame get a zero row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PRE_BLOCK) void k_feat_bwd_gauss(int P, int C, const Meta* __restrict__ meta, const int* __restrict__ radii, const GeomState g,
                                                              const float* __restrict__ feat_rows, float* __restrict__ dL_dfeatures, int accumulate)
{
    const int idx = blockIdx.x * PRE_BLOCK + threadIdx.x;
    if (idx >= P) return;
    const bool live = !(__builtin_nontemporal_load(&meta->error) & META_ERR_CAPACITY) && radii[idx] > 0;
    if (!live && accumulate) return;
    const uint32_t tiles = live ? g.tiles_touched[idx] : 0u, off = live ? g.offsets[idx] : 0u;
    float* o = dL_dfeatures + (size_t)idx * C;
    for (int c = 0; c < C; c++) {
        float sum = 0.f;
        for (uint32_t k = 0; k < tiles; k++) sum += feat_rows[(size_t)(off + k) * C + c];
        o[c] = accumulate ? o[c] + sum : sum;
    }
}

// ---------------------------------------------------------------------------------------------
// k_feat_bwd_gauss_views: k_feat_bwd_gauss for the views of a batch (read the comment of k_depth_bwd_gauss_views in tgs_depth.hip first: the
// same pass with a row of C floats where dz stands and no matrix).  One lane per (Gaussian, channel quad): Q = ceil(C / 4) neighbouring lanes
// share a Gaussian, lane q owns channels 4q .. 4q + 3, so a lane carries four sums whatever C is (no array indexed at run time: no scratch
// memory, and no LDS), a wave's loads of one row step are Q * 16 contiguous bytes per Gaussian and its stores cover whole rows of dL_dfeatures.
// Per channel: the rows of a view in row order into a sum of the view's own, the views of the chunk in ascending index, then ONE store
// (accumulate == 0: every row of the range is written, a Gaussian live in no view gets exact zeros) or one read-modify-write (a Gaussian live
// in no view is left alone) per Gaussian and chunk.  No atomics, a fixed order: two runs give the same bits, and so do the two load widths.
// Load-latency bound like the depth kernel: the first step of EVERY view of the chunk (radii / tiles_touched / offsets; the Q lanes of a
// Gaussian read the same words, one request) is issued before any row is read, and a view's rows are fetched four at a time in front of
// their four additions.  A Gaussian's rows in a view are tiles * C contiguous floats (offsets is a prefix sum, the row stride is C).
// VEC: C % 4 == 0 and the scratch of every view of the chunk and dL_dfeatures 16-byte aligned (the host checks): one 16-byte access per lane
// and row; otherwise scalar accesses, the channels behind C - 1 read as 0 and are not stored.  A view's meta word is uniform.
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float* __restrict__ p, int n)
{
    if (VEC) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], n > 1 ? p[1] : 0.f, n > 2 ? p[2] : 0.f, n > 3 ? p[3] : 0.f);
}
__device__ __forceinline__ void add_quad(float4& s, const float4 x) { s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w; }

template <bool VEC>
__global__ __launch_bounds__(PRE_BLOCK) void k_feat_bwd_gauss_views(int first, int end, int C, uint32_t Q, const FeatViews fv, float* __restrict__ dL_dfeatures,
                                                                    int accumulate)
{
    const uint32_t t = blockIdx.x * (uint32_t)PRE_BLOCK + threadIdx.x;      // (the host keeps count * Q below 2^32)
    const uint32_t g = t / Q;
    if (g >= (uint32_t)(end - first)) return;
    const int idx = first + (int)g, c0 = 4 * (int)(t - g * Q), nq = C - c0;
    uint32_t tiles[BATCH_VIEWS], off[BATCH_VIEWS];
#pragma unroll
    for (int k = 0; k < BATCH_VIEWS; k++) {
        tiles[k] = 0; off[k] = 0;
        if (k < fv.n) {
            const FeatView& w = fv.v[k];
            // a rejected frame contributes nothing (and its offsets may point past its capacity: they are not followed)
            const bool live = !(__builtin_nontemporal_load(&w.meta->error) & META_ERR_CAPACITY) && w.radii[idx] > 0;
            if (live) { tiles[k] = w.tiles_touched[idx]; off[k] = w.offsets[idx]; }
        }
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    bool any = false;
#pragma unroll
    for (int k = 0; k < BATCH_VIEWS; k++) {
        if (k < fv.n && tiles[k] > 0) {
            const float* row = fv.v[k].rows + (size_t)off[k] * C + c0;
            const uint32_t n = tiles[k];
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            uint32_t r = 0;
            for (; r + 4 <= n; r += 4, row += 4 * (size_t)C) {
                const float4 x0 = load_quad<VEC>(row, nq), x1 = load_quad<VEC>(row + C, nq), x2 = load_quad<VEC>(row + 2 * (size_t)C, nq),
                             x3 = load_quad<VEC>(row + 3 * (size_t)C, nq);
                add_quad(s, x0); add_quad(s, x1); add_quad(s, x2); add_quad(s, x3);
            }
            for (; r < n; r++, row += C) add_quad(s, load_quad<VEC>(row, nq));
            add_quad(acc, s);
            any = true;
        }
    }
    if (!any && accumulate) return;
    float* o = dL_dfeatures + (size_t)idx * C + c0;
    if (VEC) {
        float4 v = acc;
        if (accumulate) { v = *reinterpret_cast<const float4*>(o); add_quad(v, acc); }
        *reinterpret_cast<float4*>(o) = v;
    } else {
        const float a[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int c = 0; c < 4; c++) if (c < nq) o[c] = accumulate ? o[c] + a[c] : a[c];
    }
}

// ---------------------------------------------------------------------------------------------
// host launchers: one launch per group of FGROUP channels, the narrow kernel for a group of 1 .. 4
// ---------------------------------------------------------------------------------------------
// out[C * N] <- 0, then the tiles with instances (at most T workgroups have work)
void launch_feat_fwd(hipStream_t st, const ImgState& s, const BinState& b, int W, int H, uint32_t gx, uint32_t T, int P, int C, const float* features, float* out)
{
    (void)hipMemsetAsync(out, 0, (size_t)C * W * H * sizeof(float), st);
    if (T == 0) return;
    for (int c0 = 0; c0 < C; c0 += FGROUP) {
        const int nc = C - c0 < FGROUP ? C - c0 : FGROUP;
        if (nc <= 4) hipLaunchKernelGGL(k_feat_fwd<4>, dim3(T), dim3(256), 0, st, s, b, W, H, gx, (uint32_t)P, C, c0, nc, features, out);
        else hipLaunchKernelGGL(k_feat_fwd<8>, dim3(T), dim3(256), 0, st, s, b, W, H, gx, (uint32_t)P, C, c0, nc, features, out);
    }
}
// tiles: leading entries of tile_order that can hold instances (launch_render_bwd's).  feat_rows[R * C] <- 0 first: rows the kernels do not visit read as 0.
void launch_feat_bwd(hipStream_t st, const ImgState& s, const BinState& b, int W, int H, uint32_t gx, uint32_t tiles, size_t R, int P, int C, const float* features,
                     const float* dL_dmap, float* feat_rows)
{
    (void)hipMemsetAsync(feat_rows, 0, R * C * sizeof(float), st);
    if (tiles == 0) return;
    for (int c0 = 0; c0 < C; c0 += FGROUP) {
        const int nc = C - c0 < FGROUP ? C - c0 : FGROUP;
        if (nc <= 4) hipLaunchKernelGGL(k_feat_bwd<4>, dim3(tiles), dim3(256), 0, st, s, b, W, H, gx, (uint32_t)P, C, c0, nc, features, dL_dmap, feat_rows);
        else hipLaunchKernelGGL(k_feat_bwd<8>, dim3(tiles), dim3(256), 0, st, s, b, W, H, gx, (uint32_t)P, C, c0, nc, features, dL_dmap, feat_rows);
    }
}
void launch_feat_bwd_gauss(hipStream_t st, int P, int C, const Meta* meta, const int* radii, const GeomState& g, const float* feat_rows, float* dL_dfeatures, int accumulate)
{
    hipLaunchKernelGGL(k_feat_bwd_gauss, dim3((unsigned)n_blocks((size_t)P)), dim3(PRE_BLOCK), 0, st, P, C, meta, radii, g, feat_rows, dL_dfeatures, accumulate);
}
// Gaussians [first, first + count) of P, the views of one chunk; vec: the 16-byte accesses are allowed (C % 4 == 0, everything 16-byte aligned)
void launch_feat_bwd_gauss_views(hipStream_t st, int first, int count, int C, const FeatViews& fv, float* dL_dfeatures, int accumulate, bool vec)
{
    if (count <= 0 || fv.n <= 0) return;
    const uint32_t Q = (uint32_t)(C + 3) / 4;
    const dim3 grid((unsigned)n_blocks((size_t)count * Q)), blk(PRE_BLOCK);
    if (vec) hipLaunchKernelGGL(k_feat_bwd_gauss_views<true>, grid, blk, 0, st, first, first + count, C, Q, fv, dL_dfeatures, accumulate);
    else hipLaunchKernelGGL(k_feat_bwd_gauss_views<false>, grid, blk, 0, st, first, first + count, C, Q, fv, dL_dfeatures, accumulate);
}

}  // namespace tgs
