// tgs_mesh_sdf.hip -- signed distance from points to a triangle mesh, for gfx950: the target of the geometry stage's shape initialisation
// (tetgs_spatial/models/geometry/implicit_sdf.py :231-239, where a CPU k-d tree behind two copies answers it).  Plain HIP, wave64, one lane per
// point.  include/tgs_raster.h ("mesh signed distance") has the rules in full; tests/mesh_sdf_ref.py restates them.
//
//   tgs_meshsdf_build        on the host, no device call: the bounding-volume tree in depth-first order (tgs_mesh_sdf.hpp, build_tree)
//   tgs_meshsdf_query        k_meshsdf_tree (mode 0): per lane three walks over the depth-first layout without a stack -- down to the nearest
//                            leaf, the distance walk that prunes by the box's lower bound, the parity walk of the three rays;
//                            k_meshsdf_brute (mode 1): every face in the caller's order, the on-device cross-check and the path for tiny meshes
//   tgs_meshsdf_query_host   the same walks and pair functions compiled for the CPU (include/tgs_raster_testing.h)
//
// No per-lane array (no scratch), no atomics; every loop is bounded by the node count, the face count or the depth bound; a lane writes its own
// outputs, so two runs give the same bits, and mode 0 gives the bits of mode 1.
#include "tgs_device.hpp"
#include "tgs_mesh_sdf.hpp"
#include "../../include/tgs_raster.h"
#include "../../include/tgs_raster_testing.h"

#include <cstdio>

namespace tgs {

constexpr int SDF_BLOCK = 64;                  // one wave per workgroup: the walks diverge, and a workgroup is done when its slowest lane is

__global__ void __launch_bounds__(SDF_BLOCK) k_meshsdf_tree(const void* tree, int F, long long N, const float* points, int sign,
                                                            float* out_sdf, int32_t* out_face, float* out_closest, uint8_t* out_inside)
{
    const long long n = (long long)blockIdx.x * SDF_BLOCK + threadIdx.x;
    if (n >= N) return;
    msdf::point_tree(tree, F, points, n, sign != 0, out_sdf, out_face, out_closest, out_inside);
}

template <typename Index>
__global__ void __launch_bounds__(SDF_BLOCK) k_meshsdf_brute(int V, int F, const float* vertices, const Index* faces, long long N, const float* points, int sign,
                                                             float* out_sdf, int32_t* out_face, float* out_closest, uint8_t* out_inside)
{
    const long long n = (long long)blockIdx.x * SDF_BLOCK + threadIdx.x;
    if (n >= N) return;
    msdf::point_brute(V, F, vertices, faces, points, n, sign != 0, out_sdf, out_face, out_closest, out_inside);
}

static int refuse(const char* entry, const char* what)
{
    static thread_local char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    return set_error(TGS_ERR_INVALID, msg);
}

}  // namespace tgs

extern "C" {

size_t tgs_meshsdf_tree_bytes(int F)
{
    return F < 1 || F > tgs::msdf::MAX_FACES ? 0 : tgs::msdf::tree_bytes((size_t)F);
}

int tgs_meshsdf_max_faces(void) { return tgs::msdf::MAX_FACES; }

int tgs_meshsdf_build(int V, int F, const float* vertices, const void* faces, int faces_is_int64, void* tree, size_t tree_bytes)
{
    using namespace tgs;
    if (const char* bad = msdf::build_tree(V, F, vertices, faces, faces_is_int64, tree, tree_bytes)) return refuse("tgs_meshsdf_build", bad);
    return TGS_OK;
}

int tgs_meshsdf_query(void* stream, const void* tree, size_t tree_bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, int64_t N,
                      const float* points, int mode, float* out_sdf, int32_t* out_face, float* out_closest, uint8_t* out_inside)
{
    using namespace tgs;
    if (const char* bad = msdf::check_query(tree, tree_bytes, V, F, vertices, faces, faces_is_int64, (long long)N, points, mode)) return refuse("tgs_meshsdf_query", bad);
    if (N > (int64_t)0x7fffffff * SDF_BLOCK) return refuse("tgs_meshsdf_query", "N above 2^31 - 1 workgroups of 64 points");
    if (N == 0) return TGS_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + SDF_BLOCK - 1) / SDF_BLOCK)), block(SDF_BLOCK);
    const int sign = out_sdf || out_inside;
    if (mode == 0) hipLaunchKernelGGL(k_meshsdf_tree, grid, block, 0, st, tree, F, (long long)N, points, sign, out_sdf, out_face, out_closest, out_inside);
    else if (faces_is_int64) hipLaunchKernelGGL(k_meshsdf_brute<int64_t>, grid, block, 0, st, V, F, vertices, (const int64_t*)faces, (long long)N, points, sign, out_sdf, out_face, out_closest, out_inside);
    else hipLaunchKernelGGL(k_meshsdf_brute<int32_t>, grid, block, 0, st, V, F, vertices, (const int32_t*)faces, (long long)N, points, sign, out_sdf, out_face, out_closest, out_inside);
    return hip_status("tgs_meshsdf_query");
}

int tgs_meshsdf_query_host(const void* tree, size_t tree_bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, int64_t N,
                           const float* points, int mode, float* out_sdf, int32_t* out_face, float* out_closest, uint8_t* out_inside)
{
    using namespace tgs;
    if (const char* bad = msdf::query_host(tree, tree_bytes, V, F, vertices, faces, faces_is_int64, (long long)N, points, mode, out_sdf, out_face, out_closest, out_inside))
        return refuse("tgs_meshsdf_query_host", bad);
    return TGS_OK;
}

}  // extern "C"
