// tgs_mesh_rays.hip -- rays against a triangle mesh, for gfx950: the first operation of the editing pipeline (mesh_localization.py :150-167 and
// tetgs_inpainter/mask_mesh_0822.py :209-237, where open3d's RaycastingScene answers it on the CPU and a Python set collects the faces).  Plain HIP,
// wave64, one lane per ray.  include/tgs_raster.h ("mesh ray casting") has the rules in full; tests/mesh_rays_ref.py restates them.
//
//   tgs_meshrays_cast            k_meshrays_tree (mode 0): the mesh signed distance's tree in depth-first order with the skip links, without a stack,
//                                into a box when the slab test in double says the ray reaches it before the best hit so far;
//                                k_meshrays_brute (mode 1): every face in the caller's order, the on-device cross-check
//   tgs_meshrays_occluded        the same two walks, ended at the first face with a hit in [tnear, tfar]
//   tgs_meshrays_*_host          the same walks and pair functions compiled for the CPU (include/tgs_mesh_rays_testing.h)
//
// No per-lane array (no scratch), no atomics, no LDS; every loop is bounded by the node count or the face count; a lane writes its own outputs, and
// the one shared output, out_hit_faces, takes plain stores of the value 1: two runs give the same bits, and mode 0 gives the bits of mode 1.
#include "tgs_device.hpp"
#include "tgs_mesh_rays.hpp"
#include "../../include/tgs_raster.h"
#include "../../include/tgs_raster_testing.h"

#include <cstdio>

namespace tgs {

constexpr int RAYS_BLOCK = 64;                 // one wave per workgroup: the walks diverge, and a workgroup is done when its slowest lane is

__global__ void __launch_bounds__(RAYS_BLOCK) k_meshrays_tree(const void* tree, int F, long long N, const float* rays, float* out_t, int32_t* out_face, int32_t* out_geometry,
                                                              float* out_uv, float* out_normal, uint8_t* out_hit_faces)
{
    const long long n = (long long)blockIdx.x * RAYS_BLOCK + threadIdx.x;
    if (n >= N) return;
    mrays::cast_tree(tree, F, rays, n, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
}

template <typename Index>
__global__ void __launch_bounds__(RAYS_BLOCK) k_meshrays_brute(int V, int F, const float* vertices, const Index* faces, long long N, const float* rays, float* out_t, int32_t* out_face,
                                                               int32_t* out_geometry, float* out_uv, float* out_normal, uint8_t* out_hit_faces)
{
    const long long n = (long long)blockIdx.x * RAYS_BLOCK + threadIdx.x;
    if (n >= N) return;
    mrays::cast_brute(V, F, vertices, faces, rays, n, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
}

__global__ void __launch_bounds__(RAYS_BLOCK) k_meshrays_occluded_tree(const void* tree, int F, long long N, const float* rays, float tnear, float tfar, uint8_t* out_occluded)
{
    const long long n = (long long)blockIdx.x * RAYS_BLOCK + threadIdx.x;
    if (n >= N) return;
    mrays::occluded_tree(tree, F, rays, n, (double)tnear, (double)tfar, out_occluded);
}

template <typename Index>
__global__ void __launch_bounds__(RAYS_BLOCK) k_meshrays_occluded_brute(int V, int F, const float* vertices, const Index* faces, long long N, const float* rays, float tnear, float tfar,
                                                                        uint8_t* out_occluded)
{
    const long long n = (long long)blockIdx.x * RAYS_BLOCK + threadIdx.x;
    if (n >= N) return;
    mrays::occluded_brute(V, F, vertices, faces, rays, n, (double)tnear, (double)tfar, out_occluded);
}

static int refuse_rays(const char* entry, const char* what)
{
    static thread_local char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    return set_error(TGS_ERR_INVALID, msg);
}

}  // namespace tgs

extern "C" {

int tgs_meshrays_cast(void* stream, const void* tree, size_t tree_bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, int64_t N, const float* rays,
                      int mode, float* out_t, int32_t* out_face, int32_t* out_geometry, float* out_uv, float* out_normal, uint8_t* out_hit_faces)
{
    using namespace tgs;
    if (const char* bad = mrays::check_cast(tree, tree_bytes, V, F, vertices, faces, faces_is_int64, (long long)N, rays, mode)) return refuse_rays("tgs_meshrays_cast", bad);
    if (N > (int64_t)0x7fffffff * RAYS_BLOCK) return refuse_rays("tgs_meshrays_cast", "N above 2^31 - 1 workgroups of 64 rays");
    if (N == 0) return TGS_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + RAYS_BLOCK - 1) / RAYS_BLOCK)), block(RAYS_BLOCK);
    if (mode == 0) hipLaunchKernelGGL(k_meshrays_tree, grid, block, 0, st, tree, F, (long long)N, rays, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
    else if (faces_is_int64)
        hipLaunchKernelGGL(k_meshrays_brute<int64_t>, grid, block, 0, st, V, F, vertices, (const int64_t*)faces, (long long)N, rays, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
    else
        hipLaunchKernelGGL(k_meshrays_brute<int32_t>, grid, block, 0, st, V, F, vertices, (const int32_t*)faces, (long long)N, rays, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces);
    return hip_status("tgs_meshrays_cast");
}

int tgs_meshrays_occluded(void* stream, const void* tree, size_t tree_bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, int64_t N, const float* rays,
                          float tnear, float tfar, int mode, uint8_t* out_occluded)
{
    using namespace tgs;
    if (const char* bad = mrays::check_occluded(tree, tree_bytes, V, F, vertices, faces, faces_is_int64, (long long)N, rays, tnear, tfar, mode, out_occluded))
        return refuse_rays("tgs_meshrays_occluded", bad);
    if (N > (int64_t)0x7fffffff * RAYS_BLOCK) return refuse_rays("tgs_meshrays_occluded", "N above 2^31 - 1 workgroups of 64 rays");
    if (N == 0) return TGS_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + RAYS_BLOCK - 1) / RAYS_BLOCK)), block(RAYS_BLOCK);
    if (mode == 0) hipLaunchKernelGGL(k_meshrays_occluded_tree, grid, block, 0, st, tree, F, (long long)N, rays, tnear, tfar, out_occluded);
    else if (faces_is_int64) hipLaunchKernelGGL(k_meshrays_occluded_brute<int64_t>, grid, block, 0, st, V, F, vertices, (const int64_t*)faces, (long long)N, rays, tnear, tfar, out_occluded);
    else hipLaunchKernelGGL(k_meshrays_occluded_brute<int32_t>, grid, block, 0, st, V, F, vertices, (const int32_t*)faces, (long long)N, rays, tnear, tfar, out_occluded);
    return hip_status("tgs_meshrays_occluded");
}

int tgs_meshrays_cast_host(const void* tree, size_t tree_bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, int64_t N, const float* rays, int mode,
                           float* out_t, int32_t* out_face, int32_t* out_geometry, float* out_uv, float* out_normal, uint8_t* out_hit_faces)
{
    using namespace tgs;
    if (const char* bad = mrays::cast_host(tree, tree_bytes, V, F, vertices, faces, faces_is_int64, (long long)N, rays, mode, out_t, out_face, out_geometry, out_uv, out_normal, out_hit_faces))
        return refuse_rays("tgs_meshrays_cast_host", bad);
    return TGS_OK;
}

int tgs_meshrays_occluded_host(const void* tree, size_t tree_bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, int64_t N, const float* rays,
                               float tnear, float tfar, int mode, uint8_t* out_occluded)
{
    using namespace tgs;
    if (const char* bad = mrays::occluded_host(tree, tree_bytes, V, F, vertices, faces, faces_is_int64, (long long)N, rays, tnear, tfar, mode, out_occluded))
        return refuse_rays("tgs_meshrays_occluded_host", bad);
    return TGS_OK;
}

}  // extern "C"
