/*
 * tgs_mesh_sdf_testing.h -- TEST-ONLY entry point of libtgs_raster.so for the mesh signed distance (tgs_raster.h, "mesh signed distance").  NOT part of
 * the drop-in boundary.  Included by tgs_raster_testing.h; it stands in a file of its own because that header's own declarations are the
 * process- / thread-wide shims of rounds 1-2 and nothing else.
 */
#ifndef TGS_MESH_SDF_TESTING_H
#define TGS_MESH_SDF_TESTING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The host twin of tgs_meshsdf_query: the same walks and the same per-pair functions (csrc/tgs_mesh_sdf.hpp) compiled for the CPU, every pointer
 * a HOST pointer, the points one after the other.  It makes no device call, so the tree's logic is tested without a device.  The same
 * refusals as tgs_meshsdf_query; a tree whose header was not written by tgs_meshsdf_build for this F is refused with TGS_ERR_INVALID (-1) too. */
int tgs_meshsdf_query_host(const void* tree, size_t tree_bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, int64_t N,
                           const float* points, int mode, float* out_sdf, int32_t* out_face, float* out_closest, uint8_t* out_inside);

#ifdef __cplusplus
}
#endif
#endif /* TGS_MESH_SDF_TESTING_H */
