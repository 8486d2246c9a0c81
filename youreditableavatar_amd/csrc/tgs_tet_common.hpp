// tgs_tet_common.hpp -- what the kernels over tetrahedral grids share (tgs_marching_tets.hip, tgs_tet_grid.hip): a tetrahedron's row load, its
// range check and the alignment the load needs.  The scans, the run bounds, the run sort and the binary search are tgs_runs.hpp, which is not
// about tetrahedra and is included here.
#pragma once
#include "tgs_runs.hpp"

namespace tgs {

#ifdef __HIPCC__
template <typename Idx>
__device__ __forceinline__ void mt_load_tet(const Idx* __restrict__ tet, size_t f, long long t[4])
{
    if constexpr (sizeof(Idx) == 4) {
        const int4 r = reinterpret_cast<const int4*>(tet)[f];
        t[0] = r.x; t[1] = r.y; t[2] = r.z; t[3] = r.w;
    } else {
        const longlong2 r0 = reinterpret_cast<const longlong2*>(tet)[2 * f], r1 = reinterpret_cast<const longlong2*>(tet)[2 * f + 1];
        t[0] = r0.x; t[1] = r0.y; t[2] = r1.x; t[3] = r1.y;
    }
}
__device__ __forceinline__ bool mt_in_range(const long long t[4], int N)
{
    return (unsigned long long)t[0] < (unsigned long long)N && (unsigned long long)t[1] < (unsigned long long)N &&
           (unsigned long long)t[2] < (unsigned long long)N && (unsigned long long)t[3] < (unsigned long long)N;
}
static inline bool mt_aligned(const void* tet) { return ((uintptr_t)tet & 15u) == 0; }              // rows are loaded as 16-byte vectors
#endif

}  // namespace tgs
