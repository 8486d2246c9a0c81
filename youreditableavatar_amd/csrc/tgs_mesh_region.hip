// tgs_mesh_region.hip -- face-selection morphology and connected components on a triangle mesh, for gfx950: what the painting stage takes from
// pymeshlab in refine_region and gen_editing_region_mask (mesh_localization.py :34-67, :133-148): apply_selection_dilatation,
// apply_selection_erosion, the delete and compact behind them, and meshing_remove_connected_component_by_face_number.  Plain HIP, wave64, one
// lane per face.  include/tgs_raster.h ("mesh regions") has the rules in full; tests/mesh_region_ref.py restates them.
//
//   tgs_meshregion_morph       k_region_begin, then per iteration k_region_mark and k_region_select, then k_region_vertices: the iterations are
//                              queued back to back, nothing is read back.  The vertex flags are words that hold the NUMBER of the iteration
//                              that marked them, so they are cleared once per call and not once per iteration
//   tgs_meshregion_components_begin / _rounds / _finish
//                              the undirected edges of the selected faces in the table of tgs_edge_set.hpp, one label per slot; a round pushes
//                              every face's label to its three slots (atomicMin), pulls the least, hooks the face's old label to it, and
//                              jumps label[f] = label[label[f]] twice; the caller reads `changed` (the last round's) back between calls of _rounds
//
// Integer atomics and plain stores of one value only; a label only falls and ends as the least face index of its component whatever the order
// of the lanes: two runs give the same bits.  A face with an index outside [0, V) is never selected and its indices are never used as addresses.
#define TGS_EDGE_SET_TABLE_ONLY
#include "tgs_edge_set.hpp"
#include "../../include/tgs_raster.h"

#include <cstdio>

namespace tgs {

constexpr int RG_BLOCK = 256;
constexpr int REGION_MAX_FACES = (1 << 28) - 1;
constexpr int REGION_MAX_ITERATIONS = 1 << 20;
constexpr uint32_t NO_SLOT = 0xffffffffu;
constexpr int32_t NO_LABEL = 0x7f7f7f7f;                        // what a memset of 0x7f leaves: above every face index

struct Tri { int a, b, c; bool ok; };
__device__ __forceinline__ Tri load_tri(const int32_t* __restrict__ faces, int f, int V)
{
    Tri t{faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2], false};
    t.ok = (unsigned)t.a < (unsigned)V && (unsigned)t.b < (unsigned)V && (unsigned)t.c < (unsigned)V;
    return t;
}

// sel <- the caller's selection, without the faces that have an index outside [0, V)
__global__ void __launch_bounds__(RG_BLOCK) k_region_begin(int V, int F, const int32_t* __restrict__ faces, const uint8_t* __restrict__ sel_in, uint8_t* __restrict__ sel)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    sel[f] = (sel_in[f] != 0 && load_tri(faces, f, V).ok) ? 1 : 0;
}
// iteration `epoch` (>= 1): a selected face writes the epoch to its vertices' words of `has_sel`, an unselected one (erosion only) to `has_unsel`
template <bool ERODE>
__global__ void __launch_bounds__(RG_BLOCK) k_region_mark(int V, int F, const int32_t* __restrict__ faces, const uint8_t* __restrict__ sel, uint32_t epoch,
                                                          uint32_t* __restrict__ has_sel, uint32_t* __restrict__ has_unsel)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const Tri t = load_tri(faces, f, V);
    if (!t.ok) return;                                           // touches no vertex
    if (sel[f]) { has_sel[t.a] = epoch; has_sel[t.b] = epoch; has_sel[t.c] = epoch; }
    else if (ERODE) { has_unsel[t.a] = epoch; has_unsel[t.b] = epoch; has_unsel[t.c] = epoch; }
}
// loose (dilation): any of the three vertices is marked; strict (erosion): all three have a selected face and no unselected one
template <bool ERODE>
__global__ void __launch_bounds__(RG_BLOCK) k_region_select(int V, int F, const int32_t* __restrict__ faces, uint8_t* __restrict__ sel, uint32_t epoch,
                                                            const uint32_t* __restrict__ has_sel, const uint32_t* __restrict__ has_unsel)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const Tri t = load_tri(faces, f, V);
    bool on = false;
    if (t.ok) {
        if (ERODE) on = has_sel[t.a] == epoch && has_sel[t.b] == epoch && has_sel[t.c] == epoch && has_unsel[t.a] != epoch && has_unsel[t.b] != epoch && has_unsel[t.c] != epoch;
        else on = has_sel[t.a] == epoch || has_sel[t.b] == epoch || has_sel[t.c] == epoch;
    }
    sel[f] = on ? 1 : 0;
}
// vertex_mask (cleared in front): the vertices some selected face references
__global__ void __launch_bounds__(RG_BLOCK) k_region_vertices(int V, int F, const int32_t* __restrict__ faces, const uint8_t* __restrict__ sel, uint8_t* __restrict__ vertex_mask)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F || !sel[f]) return;
    const Tri t = load_tri(faces, f, V);
    if (!t.ok) return;
    vertex_mask[t.a] = 1; vertex_mask[t.b] = 1; vertex_mask[t.c] = 1;
}

// ---- components ----
struct CompState {
    unsigned long long* keys;     // [cap] the edge table
    int32_t* elabel;              // [cap] the least label pushed to the slot
    uint32_t* slots;              // [3 F] a face's three slots, NO_SLOT for a side (i, i) and for an unselected face
    int32_t* count;               // [F] faces per label
    int32_t* changed;             // [1] a round lowered a label
    size_t cap;
};
__host__ __device__ inline size_t comp_capacity(size_t F)                      // a power of two >= 4 F: at most 3 F keys, never above 3/4 full
{
    size_t cap = 64;
    while (cap < 4 * F) cap <<= 1;
    return cap;
}
__host__ __device__ inline size_t comp_carve(CompState& s, char* base, size_t F)
{
    char* p = base;
    s.cap = comp_capacity(F);
    carve(p, s.keys, s.cap); carve(p, s.elabel, s.cap); carve(p, s.slots, 3 * F); carve(p, s.count, F); carve(p, s.changed, 64);
    return (size_t)(p - base) + 256;
}

__global__ void __launch_bounds__(RG_BLOCK) k_comp_begin(int V, int F, const int32_t* __restrict__ faces, const uint8_t* __restrict__ sel, int32_t* __restrict__ label, CompState s)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const Tri t = load_tri(faces, f, V);
    const bool on = sel[f] != 0 && t.ok;
    label[f] = on ? f : -1;
    const int u[3] = {t.a, t.b, t.c}, w[3] = {t.b, t.c, t.a};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        uint32_t slot = NO_SLOT;
        if (on && u[i] != w[i]) {
            bool claimed;
            const size_t at = edge_insert(s.keys, s.cap, edge_key(min(u[i], w[i]), max(u[i], w[i])), claimed);
            if (at != EDGE_ABSENT) slot = (uint32_t)at;
        }
        s.slots[3 * (size_t)f + i] = slot;
    }
}
__global__ void __launch_bounds__(RG_BLOCK) k_comp_push(int F, const int32_t* __restrict__ label, CompState s)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int32_t l = label[f];
    if (l < 0) return;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const uint32_t slot = s.slots[3 * (size_t)f + i];
        if (slot != NO_SLOT && s.elabel[slot] > l) atomicMin(&s.elabel[slot], l);
    }
}
// m = the least label on the face's slots; below the face's own: the own label's face learns it too (the hook), so that everything that
// points there follows in the jumps
__global__ void __launch_bounds__(RG_BLOCK) k_comp_pull(int F, int32_t* __restrict__ label, CompState s)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int32_t l = label[f];
    if (l < 0 || l >= F) return;
    int32_t m = l;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const uint32_t slot = s.slots[3 * (size_t)f + i];
        if (slot != NO_SLOT) m = min(m, s.elabel[slot]);
    }
    if (m < l) {                                                  // 0 <= m < l <= f < F: both are faces of this component
        atomicMin(&label[l], m);
        atomicMin(&label[f], m);
        *s.changed = 1;
    }
}
__global__ void __launch_bounds__(RG_BLOCK) k_comp_jump(int F, int32_t* __restrict__ label, CompState s)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int32_t l = label[f];
    if (l < 0 || l >= F) return;
    const int32_t ll = label[l];                                  // (another lane may be lowering it: any value it has held is a face of the component)
    if (ll >= 0 && ll < l) { atomicMin(&label[f], ll); *s.changed = 1; }
}
__global__ void __launch_bounds__(RG_BLOCK) k_comp_count(int F, const int32_t* __restrict__ label, CompState s)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int32_t l = label[f];
    if (l >= 0 && l < F) atomicAdd(&s.count[l], 1);
}
__global__ void __launch_bounds__(RG_BLOCK) k_comp_size(int F, const int32_t* __restrict__ label, int32_t* __restrict__ size, CompState s)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int32_t l = label[f];
    size[f] = (l >= 0 && l < F) ? s.count[l] : 0;
}

static int rg_refuse(const char* entry, const char* what)
{
    static thread_local char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    return set_error(TGS_ERR_INVALID, msg);
}
static const char* rg_check_mesh(int V, int F, const void* faces)
{
    if (V < 0) return "V >= 0 is required";
    if (F < 0 || F > REGION_MAX_FACES) return "0 <= F <= 2^28 - 1 is required";
    if (F && !faces) return "faces must be non-NULL";
    return nullptr;
}
static dim3 rg_grid(int F) { return dim3((unsigned)((F + RG_BLOCK - 1) / RG_BLOCK)); }

}  // namespace tgs

extern "C" {

size_t tgs_meshregion_workspace_bytes(int V, int F)
{
    if (V < 0 || F < 0 || F > tgs::REGION_MAX_FACES) return 0;
    return 2 * (size_t)V * sizeof(uint32_t) + 512;
}

int tgs_meshregion_morph(void* stream, int V, int F, const int32_t* faces, const uint8_t* sel_in, int dilate_iter, int erode_iter, uint8_t* sel_out, uint8_t* vertex_mask,
                         void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    if (const char* bad = rg_check_mesh(V, F, faces)) return rg_refuse("tgs_meshregion_morph", bad);
    if (dilate_iter < 0 || erode_iter < 0 || dilate_iter > REGION_MAX_ITERATIONS || erode_iter > REGION_MAX_ITERATIONS)
        return rg_refuse("tgs_meshregion_morph", "0 <= dilate_iter, erode_iter <= 2^20 is required");
    if (F && (!sel_in || !sel_out)) return rg_refuse("tgs_meshregion_morph", "sel_in and sel_out must be non-NULL");
    if (sel_in == sel_out && F) return rg_refuse("tgs_meshregion_morph", "sel_out must not be sel_in");
    if (!workspace || workspace_bytes < tgs_meshregion_workspace_bytes(V, F)) return rg_refuse("tgs_meshregion_morph", "the workspace is smaller than tgs_meshregion_workspace_bytes says");
    hipStream_t st = (hipStream_t)stream;
    if (vertex_mask && V) { if (hipMemsetAsync(vertex_mask, 0, (size_t)V, st) != hipSuccess) return hip_status("tgs_meshregion_morph"); }
    if (F == 0) return TGS_OK;
    char* p = (char*)workspace;
    uint32_t *has_sel, *has_unsel;
    carve(p, has_sel, (size_t)V); carve(p, has_unsel, (size_t)V);
    if (V && (dilate_iter || erode_iter)) { if (hipMemsetAsync(workspace, 0, tgs_meshregion_workspace_bytes(V, F), st) != hipSuccess) return hip_status("tgs_meshregion_morph"); }
    const dim3 grid = rg_grid(F), block(RG_BLOCK);
    hipLaunchKernelGGL(k_region_begin, grid, block, 0, st, V, F, faces, sel_in, sel_out);
    uint32_t epoch = 0;
    for (int i = 0; i < dilate_iter; i++) {
        epoch++;
        hipLaunchKernelGGL(k_region_mark<false>, grid, block, 0, st, V, F, faces, (const uint8_t*)sel_out, epoch, has_sel, has_unsel);
        hipLaunchKernelGGL(k_region_select<false>, grid, block, 0, st, V, F, faces, sel_out, epoch, (const uint32_t*)has_sel, (const uint32_t*)has_unsel);
    }
    for (int i = 0; i < erode_iter; i++) {
        epoch++;
        hipLaunchKernelGGL(k_region_mark<true>, grid, block, 0, st, V, F, faces, (const uint8_t*)sel_out, epoch, has_sel, has_unsel);
        hipLaunchKernelGGL(k_region_select<true>, grid, block, 0, st, V, F, faces, sel_out, epoch, (const uint32_t*)has_sel, (const uint32_t*)has_unsel);
    }
    if (vertex_mask) hipLaunchKernelGGL(k_region_vertices, grid, block, 0, st, V, F, faces, (const uint8_t*)sel_out, vertex_mask);
    return hip_status("tgs_meshregion_morph");
}

size_t tgs_meshregion_components_workspace_bytes(int F)
{
    if (F < 0 || F > tgs::REGION_MAX_FACES) return 0;
    tgs::CompState s;
    return tgs::comp_carve(s, nullptr, (size_t)F);
}

// F rounds of plain propagation at the worst, one quiet round, and the caller's block of at most 16 rounds to see it in
int tgs_meshregion_components_max_rounds(int F) { return F < 0 || F > tgs::REGION_MAX_FACES ? 0 : F + 16; }

int tgs_meshregion_components_begin(void* stream, int V, int F, const int32_t* faces, const uint8_t* sel, int32_t* label, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    if (const char* bad = rg_check_mesh(V, F, faces)) return rg_refuse("tgs_meshregion_components_begin", bad);
    if (F && (!sel || !label)) return rg_refuse("tgs_meshregion_components_begin", "sel and label must be non-NULL");
    if (!workspace || workspace_bytes < tgs_meshregion_components_workspace_bytes(F)) return rg_refuse("tgs_meshregion_components_begin", "the workspace is smaller than tgs_meshregion_components_workspace_bytes says");
    CompState s;
    comp_carve(s, (char*)workspace, (size_t)F);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(s.keys, 0xff, s.cap * sizeof(unsigned long long), st) != hipSuccess || hipMemsetAsync(s.elabel, 0x7f, s.cap * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(s.changed, 0, 64 * sizeof(int32_t), st) != hipSuccess)
        return hip_status("tgs_meshregion_components_begin");
    if (F == 0) return TGS_OK;
    hipLaunchKernelGGL(k_comp_begin, rg_grid(F), dim3(RG_BLOCK), 0, st, V, F, faces, sel, label, s);
    return hip_status("tgs_meshregion_components_begin");
}

int tgs_meshregion_components_rounds(void* stream, int F, int32_t* label, int rounds_done, int rounds, int32_t* changed, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    if (F < 0 || F > REGION_MAX_FACES) return rg_refuse("tgs_meshregion_components_rounds", "0 <= F <= 2^28 - 1 is required");
    if (rounds < 1 || rounds > 16 || rounds_done < 0) return rg_refuse("tgs_meshregion_components_rounds", "1 <= rounds <= 16 and rounds_done >= 0 are required");
    if (rounds_done >= tgs_meshregion_components_max_rounds(F)) return rg_refuse("tgs_meshregion_components_rounds", "the cap of F + 16 rounds is reached and a label still fell: the loop ends here");
    if (!changed || (F && !label)) return rg_refuse("tgs_meshregion_components_rounds", "label and changed must be non-NULL");
    if (!workspace || workspace_bytes < tgs_meshregion_components_workspace_bytes(F)) return rg_refuse("tgs_meshregion_components_rounds", "the workspace is smaller than tgs_meshregion_components_workspace_bytes says");
    CompState s;
    comp_carve(s, (char*)workspace, (size_t)F);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = rg_grid(F), block(RG_BLOCK);
    for (int r = 0; r < rounds; r++) {
        // `changed` is the LAST round's: a whole round in which no label fell is the fixed point
        if (r == rounds - 1 && hipMemsetAsync(s.changed, 0, sizeof(int32_t), st) != hipSuccess) return hip_status("tgs_meshregion_components_rounds");
        if (F == 0) continue;
        hipLaunchKernelGGL(k_comp_push, grid, block, 0, st, F, (const int32_t*)label, s);
        hipLaunchKernelGGL(k_comp_pull, grid, block, 0, st, F, label, s);
        hipLaunchKernelGGL(k_comp_jump, grid, block, 0, st, F, label, s);
        hipLaunchKernelGGL(k_comp_jump, grid, block, 0, st, F, label, s);
    }
    if (hipMemcpyAsync(changed, s.changed, sizeof(int32_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return hip_status("tgs_meshregion_components_rounds");
    return hip_status("tgs_meshregion_components_rounds");
}

int tgs_meshregion_components_finish(void* stream, int F, const int32_t* label, int32_t* size, void* workspace, size_t workspace_bytes)
{
    using namespace tgs;
    if (F < 0 || F > REGION_MAX_FACES) return rg_refuse("tgs_meshregion_components_finish", "0 <= F <= 2^28 - 1 is required");
    if (F && (!label || !size)) return rg_refuse("tgs_meshregion_components_finish", "label and size must be non-NULL");
    if (!workspace || workspace_bytes < tgs_meshregion_components_workspace_bytes(F)) return rg_refuse("tgs_meshregion_components_finish", "the workspace is smaller than tgs_meshregion_components_workspace_bytes says");
    if (F == 0) return TGS_OK;
    CompState s;
    comp_carve(s, (char*)workspace, (size_t)F);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(s.count, 0, (size_t)F * sizeof(int32_t), st) != hipSuccess) return hip_status("tgs_meshregion_components_finish");
    hipLaunchKernelGGL(k_comp_count, rg_grid(F), dim3(RG_BLOCK), 0, st, F, label, s);
    hipLaunchKernelGGL(k_comp_size, rg_grid(F), dim3(RG_BLOCK), 0, st, F, label, size, s);
    return hip_status("tgs_meshregion_components_finish");
}

}  // extern "C"
