/*
 * tgs_mesh_rays_testing.h -- TEST-ONLY entry points of libtgs_raster.so for the mesh ray casting (tgs_raster.h, "mesh ray casting").  NOT part of the
 * drop-in boundary.  Included by tgs_raster_testing.h; it stands in a file of its own for the reason tgs_mesh_sdf_testing.h does.
 */
#ifndef TGS_MESH_RAYS_TESTING_H
#define TGS_MESH_RAYS_TESTING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The host twins of tgs_meshrays_cast and tgs_meshrays_occluded: the same walks and the same per-pair functions (csrc/tgs_mesh_rays.hpp) compiled
 * for the CPU, every pointer a HOST pointer, the rays one after the other.  They make no device call, so the walks are tested without a device.
 * The same refusals as the device entry points.  Like the lanes of the kernels, they check the tree's header per ray: a tree whose header was not
 * written by tgs_meshsdf_build for this F gives miss rows in mode 0, and the call returns TGS_OK. */
int tgs_meshrays_cast_host(const void* tree, size_t tree_bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, int64_t N, const float* rays, int mode,
                           float* out_t, int32_t* out_face, int32_t* out_geometry, float* out_uv, float* out_normal, uint8_t* out_hit_faces);
int tgs_meshrays_occluded_host(const void* tree, size_t tree_bytes, int V, int F, const float* vertices, const void* faces, int faces_is_int64, int64_t N, const float* rays,
                               float tnear, float tfar, int mode, uint8_t* out_occluded);

#ifdef __cplusplus
}
#endif
#endif /* TGS_MESH_RAYS_TESTING_H */
