// tgs_median.hip -- median depth and surface index of a finished colour frame and the median's gradient, for gfx950 (wave64).
//
//   k_median_fwd   per pixel the first blended pair after which the transmittance T falls below one half: its view-space z (median_depth),
//                  its Gaussian index (median_index) and its 1-based position in the tile's list (median_pos; 0: none)
//   k_median_bwd   dL/dz of the median entries: the upstream gradients of a tile's pixels that share a median entry, summed in a fixed order
//                  into that instance's row of a per-instance scratch.  No pair is replayed: median_pos names the row.
//   (the per-Gaussian half is k_depth_bwd_gauss of tgs_depth.hip, unchanged: the sum of a Gaussian's rows times the third row of the view
//   transform, added to dL_dmeans3D; for the views of a batch k_depth_bwd_gauss_views)
//   k_surface_votes  over the median_index maps of any number of views: per Gaussian the pixels whose surface it is, and those of them
//                  inside a mask -- integer counts, one atomic per run of equal indices in a wave
//
// The forward is k_depth_fwd's walk (tgs_depth.hip) with less to do per pair: the same geometry (256 threads per tile, one lane per pixel,
// wave w owns the 8x8-pixel quadrant w), the same staging rounds, the same replay of which pairs were blended (replay_pair_alpha, positions
// 1 .. n_contrib, the two cut-offs) and the same T <- T * (1 - alpha).  z and the index are the two words of the instance's sorted key
// (k_scatter: bits(GeomState::depth) << 32 | index).  A lane is finished at its median entry; a tile stops staging once every lane is.
// median_depth is piecewise constant in every alpha: its only derivative is 1 with respect to the z of the median entry.
// No float atomics, one writer per row: two runs give the same bits.
#include "tgs_replay.hpp"

namespace tgs {

// ---------------------------------------------------------------------------------------------
// k_median_fwd: one workgroup per tile of tile_desc (workgroups behind the tiles with instances return: the outputs are filled with
// 0 / -1 / 0 in front of the launch, which is also what a rejected frame, a tile without instances and a pixel whose T stays at or
// above one half keep).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_median_fwd(const ImgState s, const BinState b, int W, int H, uint32_t gx, float* __restrict__ out_depth,
                                                    int* __restrict__ out_index, int* __restrict__ out_pos)
{
    __shared__ float4 sA[RCHUNK + 1];
    __shared__ float4 sB[RCHUNK + 1];
    __shared__ float sZ[RCHUNK + 1];
    __shared__ uint32_t sI[RCHUNK + 1];
    __shared__ QuadLists L;
    __shared__ uint32_t wmax[4];
    __shared__ uint32_t wopen[4];                           // per wave: a lane of it has pairs left and no median entry yet

    const uint2 ff = frame_flags(s);
    if ((ff.x & META_ERR_CAPACITY) || blockIdx.x >= ff.y) return;
    const ReplayLane ln = replay_lane(s, gx, W, H);
    const int wv = ln.wv, lane = ln.lane;
    const uint32_t start = ln.start, n = ln.n;
    // positions a lane still looks at: 1 .. last_contributor; set to 0 at its median entry
    uint32_t last_contributor = ln.inside ? s.n_contrib[ln.pix_id] : 0u;
    const uint32_t qmax = min(tile_deepest(last_contributor, wmax, wv, lane), n);
    if (qmax == 0) return;
    if (threadIdx.x == 0) { sA[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f); sB[RNULL] = make_float4(0.f, 0.f, 0.f, 0.f); sZ[RNULL] = 0.f; sI[RNULL] = 0u; }

    float T = 1.0f, mz = 0.f;
    uint32_t mi = 0u, mpos = 0u;                            // mpos: 1-based list position of the median entry (0: none so far)
    for (uint32_t base = 0; base < qmax; base += RCHUNK) {
        const uint32_t cnt = min((uint32_t)RCHUNK, qmax - base);
        __syncthreads();                                    // the previous round's records have been read, its wopen words written
        if (base > 0 && (wopen[0] | wopen[1] | wopen[2] | wopen[3]) == 0u) break;      // (uniform) every lane of the tile is finished
        uint32_t qm = 0;
        if (threadIdx.x < cnt) {
            const uint32_t pos = start + base + threadIdx.x;
            const unsigned long long key = b.keys[pos];
            sA[threadIdx.x] = b.recA[pos]; sB[threadIdx.x] = b.recB[pos];
            sZ[threadIdx.x] = __uint_as_float((uint32_t)(key >> 32));
            sI[threadIdx.x] = (uint32_t)key;
            qm = block_to_quadrant_mask(__float_as_uint(b.recC[pos].y));
        }
        build_quad_lists(L, qm, wv, lane);
        __syncthreads();
        // (wave-uniform) a wave whose lanes are all finished, or have nothing in this round and behind it, skips the walk
        bool wave_open = __builtin_amdgcn_ballot_w64(last_contributor > base) != 0ull;
#pragma unroll 1
        for (int sw = 0; sw < 4 && wave_open; sw++) {       // staging waves in order: the quadrant's entries front to back
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
                        T = T * (1.f - alpha);
                        if (T < 0.5f) { mz = sZ[j[u]]; mi = sI[j[u]]; mpos = base + j[u] + 1u; last_contributor = 0u; }
                    }
                }
            }
            wave_open = __builtin_amdgcn_ballot_w64(last_contributor > base) != 0ull;
        }
        const bool more = __builtin_amdgcn_ballot_w64(last_contributor > base + cnt) != 0ull;      // (the whole wave votes: outside the lane-0 branch)
        if (lane == 0) wopen[wv] = more ? 1u : 0u;
    }
    if (ln.inside && mpos > 0u) { out_depth[ln.pix_id] = mz; out_index[ln.pix_id] = (int)mi; out_pos[ln.pix_id] = (int)mpos; }
}

// ---------------------------------------------------------------------------------------------
// k_median_bwd: one workgroup per tile with instances, one lane per pixel; no pair arithmetic.  The 256 (median_pos, g) of the tile lie in
// LDS; thread t owns its position if no lower thread has it, sums the g of every thread with that position in ascending thread order and
// stores the sum to dz_rows[slot of that instance] (zero-filled in front of the launch; a row has one writer: its tile's workgroup).
// A position beyond the tile's list (a median_pos map that is not this frame's) is ignored.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_median_bwd(const ImgState s, const BinState b, int W, int H, uint32_t gx, unsigned long long R,
                                                    const int* __restrict__ median_pos, const float* __restrict__ dL_dmedian, float* __restrict__ dz_rows)
{
    __shared__ alignas(16) uint32_t sPos[256];
    __shared__ alignas(16) float sG[256];

    const uint2 ff = frame_flags(s);
    if ((ff.x & META_ERR_CAPACITY) || blockIdx.x >= ff.y) return;
    const ReplayLane ln = replay_lane(s, gx, W, H);
    uint32_t pos = 0u;
    float g = 0.f;
    if (ln.inside) {
        const int p = median_pos[ln.pix_id];
        if (p > 0 && (uint32_t)p <= ln.n) { pos = (uint32_t)p; g = dL_dmedian[ln.pix_id]; }
    }
    sPos[threadIdx.x] = pos; sG[threadIdx.x] = g;
    __syncthreads();
    if (pos == 0u) return;
    float sum = 0.f;
    bool owner = true;
#pragma unroll 1
    for (uint32_t t0 = 0; t0 < 256u; t0 += 4u) {            // every lane reads the same words: LDS broadcasts
        const uint4 p4 = *reinterpret_cast<const uint4*>(&sPos[t0]);
        const float4 g4 = *reinterpret_cast<const float4*>(&sG[t0]);
        if (p4.x == pos) { owner = owner && t0 + 0u >= threadIdx.x; sum += g4.x; }
        if (p4.y == pos) { owner = owner && t0 + 1u >= threadIdx.x; sum += g4.y; }
        if (p4.z == pos) { owner = owner && t0 + 2u >= threadIdx.x; sum += g4.z; }
        if (p4.w == pos) { owner = owner && t0 + 3u >= threadIdx.x; sum += g4.w; }
    }
    if (!owner) return;
    const size_t at = (size_t)ln.start + pos - 1u;
    if (at >= R) return;
    const uint32_t slot = b.slot[at];
    if (slot < R) dz_rows[slot] = sum;
}

// ---------------------------------------------------------------------------------------------
// k_surface_votes: which Gaussians are the visible surface, counted over n pixels (the median_index maps of any number of views, one behind
// the other): seen[p] += pixels with index p, hits[p] += those of them whose mask byte is not zero (mask == NULL: hits is not touched).
// One lane per pixel in row-major order.  Neighbouring pixels mostly share their surface splat, so a wave issues ONE atomic per run of
// equal indices, not one per pixel: a lane whose left neighbour holds another index is the head of a run (lane 0 always is: runs end at
// the wave), the run's length is the distance to the next head in the ballot of the heads, its masked pixels are the mask ballot's bits
// within the run.  An index outside 0 .. P-1 (-1: no surface) counts for nobody.  Integer adds, their results unused: the counts do not
// depend on the order, two runs give the same bits.  Every lane of a workgroup reaches the shuffle and the ballots: no early return.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_surface_votes(int P, long long n, const int* __restrict__ index, const uint8_t* __restrict__ mask,
                                                       int* __restrict__ seen, int* __restrict__ hits)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int idx = -1;
    bool masked = false;
    if (i < n) {
        const int v = index[i];
        if (v >= 0 && v < P) { idx = v; masked = mask != nullptr && mask[i] != 0; }
    }
    const int left = __shfl_up(idx, 1);
    const bool head = lane == 0 || left != idx;
    const unsigned long long heads = __builtin_amdgcn_ballot_w64(head);
    const unsigned long long mbits = __builtin_amdgcn_ballot_w64(masked);
    if (!head || idx < 0) return;
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);      // the heads to the right of this one
    const int len = above ? __ffsll(above) : 64 - lane;                            // 1 .. 64
    const unsigned long long run = (len == 64 ? ~0ull : (1ull << len) - 1ull) << lane;
    atomicAdd(&seen[idx], len);
    if (mask != nullptr) {
        const int c = __popcll(mbits & run);
        if (c) atomicAdd(&hits[idx], c);
    }
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------
// out_depth[N] <- 0, out_index[N] <- -1, out_pos[N] <- 0, then the tiles with instances (at most T workgroups have work)
void launch_median_fwd(hipStream_t st, const ImgState& s, const BinState& b, int W, int H, uint32_t gx, uint32_t T, float* out_depth, int* out_index, int* out_pos)
{
    const size_t bytes = (size_t)W * H * sizeof(float);
    (void)hipMemsetAsync(out_depth, 0, bytes, st);
    (void)hipMemsetAsync(out_index, 0xff, bytes, st);
    (void)hipMemsetAsync(out_pos, 0, bytes, st);
    if (T > 0) hipLaunchKernelGGL(k_median_fwd, dim3(T), dim3(256), 0, st, s, b, W, H, gx, out_depth, out_index, out_pos);
}
// dz_rows[R] <- 0 first: rows that are no pixel's median entry read as 0
void launch_median_bwd(hipStream_t st, const ImgState& s, const BinState& b, int W, int H, uint32_t gx, uint32_t T, size_t R, const int* median_pos,
                       const float* dL_dmedian, float* dz_rows)
{
    (void)hipMemsetAsync(dz_rows, 0, R * sizeof(float), st);
    if (T > 0) hipLaunchKernelGGL(k_median_bwd, dim3(T), dim3(256), 0, st, s, b, W, H, gx, (unsigned long long)R, median_pos, dL_dmedian, dz_rows);
}
// seen / hits are added to: the caller zero-fills them.  n > 0, and (n + 255) / 256 fits a grid (the caller checks)
void launch_surface_votes(hipStream_t st, int P, long long n, const int* index, const uint8_t* mask, int* seen, int* hits)
{
    hipLaunchKernelGGL(k_surface_votes, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, P, n, index, mask, seen, hits);
}

}  // namespace tgs
