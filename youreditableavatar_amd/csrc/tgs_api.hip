// tgs_api.hip -- the C ABI of include/tgs_raster.h: argument checks, state-buffer carving, launches.
// Host orchestration counterpart of cuda_rasterizer/rasterizer_impl.cu:141-434.
#include "tgs_device.hpp"
#include "../../include/tgs_raster.h"
#include "../../include/tgs_raster_testing.h"   // the test-only shims are defined in this file

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace tgs {
void launch_preprocess_fwd(hipStream_t, const FwdIn&, const CamParams&, const GeomState&, const ImgState&);
void launch_preprocess_fwd_batch(hipStream_t, const FwdIn&, const FwdViews&);
void launch_scan(hipStream_t, const GeomState&, const ImgState&, uint32_t nblocks, uint32_t T, uint32_t sort_cap, unsigned long long r_capacity,
                 uint32_t tile_bound, uint32_t heavy_bound, uint32_t mid_bound, Meta* host_meta, int light);
void launch_bin_count(hipStream_t, int P, const GeomState&, const ImgState&, uint32_t gx, uint32_t T);
void launch_scatter(hipStream_t, int P, const GeomState&, const ImgState&, const BinState&, uint32_t gx, uint32_t T);
void launch_tile_sort(hipStream_t, const GeomState&, const ImgState&, const BinState&, uint32_t gx, uint32_t T, uint64_t r_bound, const Meta* m,
                      uint32_t sort_cap, uint32_t tile_bound, uint32_t heavy_bound, uint32_t mid_bound);
void launch_render_fwd(hipStream_t, const ImgState&, const BinState&, int W, int H, uint32_t gx, uint32_t T, const Meta* m, const float* bg,
                       float* out_color, uint32_t tile_bound, uint32_t mid_bound, int light);
void launch_mark_visible(hipStream_t, int P, const float* means3D, const float* view, uint8_t* present);
void launch_alpha(hipStream_t, const ImgState&, size_t N, float* out_alpha);
void launch_render_bwd(hipStream_t, const ImgState&, const BinState&, int W, int H, uint32_t gx, uint32_t tiles, const float* bg, const float* dL_dpix,
                       const float* dL_dalpha, bool deterministic, uint32_t mid_tiles, int light, uint32_t T);
void launch_preprocess_bwd(hipStream_t, const BwdIn&, const CamParams&, const GeomState&, const BinState&);
void launch_preprocess_bwd_batch(hipStream_t, const BwdIn&, const BatchViews&);
void launch_selftest_reduce36(hipStream_t, const float* in, float* out);
// tgs_depth.hip
void launch_depth_fwd(hipStream_t, const ImgState&, const BinState&, int W, int H, uint32_t gx, uint32_t T, float* out_depth);
void launch_depth_bwd(hipStream_t, const ImgState&, const BinState&, int W, int H, uint32_t gx, uint32_t tiles, size_t R, const float* dL_ddepth, float* dz_rows);
void launch_depth_bwd_gauss(hipStream_t, int P, const Meta* meta, const int* radii, const GeomState&, const float* view, const float* dz_rows, float* dL_dmean3D);
void launch_depth_bwd_gauss_views(hipStream_t, int first, int count, const DepthViews&, float* dL_dmean3D);
// tgs_feature.hip
void launch_feat_fwd(hipStream_t, const ImgState&, const BinState&, int W, int H, uint32_t gx, uint32_t T, int P, int C, const float* features, float* out);
void launch_feat_bwd(hipStream_t, const ImgState&, const BinState&, int W, int H, uint32_t gx, uint32_t tiles, size_t R, int P, int C, const float* features,
                     const float* dL_dmap, float* feat_rows);
void launch_feat_bwd_gauss(hipStream_t, int P, int C, const Meta* meta, const int* radii, const GeomState&, const float* feat_rows, float* dL_dfeatures, int accumulate);
void launch_feat_bwd_gauss_views(hipStream_t, int first, int count, int C, const FeatViews&, float* dL_dfeatures, int accumulate, bool vec);
// tgs_median.hip
void launch_median_fwd(hipStream_t, const ImgState&, const BinState&, int W, int H, uint32_t gx, uint32_t T, float* out_depth, int* out_index, int* out_pos);
void launch_median_bwd(hipStream_t, const ImgState&, const BinState&, int W, int H, uint32_t gx, uint32_t T, size_t R, const int* median_pos, const float* dL_dmedian,
                       float* dz_rows);
void launch_surface_votes(hipStream_t, int P, long long n, const int* index, const uint8_t* mask, int* seen, int* hits);
}  // namespace tgs

using namespace tgs;

static thread_local char g_err[512] = "";

#include <atomic>
#include <cstdlib>
// -1: not set by the API -> environment variable TGS_DETERMINISTIC decides (default 0)
static std::atomic<int> g_deterministic{-1};
static std::atomic<uint32_t> g_sort_cap{SORT_LDS_CAP};
static std::atomic<int> g_fwd_group{2};
static std::atomic<int> g_prune{1};
#ifndef TGS_LIGHT_TILES_DEFAULT
#define TGS_LIGHT_TILES_DEFAULT 1
#endif
static bool deterministic_mode()
{
    const int v = g_deterministic.load(std::memory_order_relaxed);
    if (v >= 0) return v != 0;
    const char* e = getenv("TGS_DETERMINISTIC");
    return e && e[0] && e[0] != '0';
}

// Everything that tunes one call (include/tgs_raster.h: tgs_options_t), resolved ONCE at the entry point and passed down by value: the
// kernels and launchers never read a global.  Fields a caller leaves at their default fall back to the test-only setters' values.
struct Opts {
    int prune;
    bool deterministic;
    int fwd_group;
    uint32_t sort_cap;
    int64_t tile_bound, heavy_bound, mid_bound;
    int light;
};
static thread_local int64_t t_tile_bound = 0;               // tgs_set_tile_bound (test-only shim): default tile bound of this thread's calls without options
// batch: the *_views entry points (several views in flight on several streams), where the light groups pay: +4 % on the 8-view step of
// config 3 (2.16 -> 2.07 ms), while a view that has the GPU to itself loses 1-2 % (its kernels end with the light groups' ~10-us tail)
static Opts resolve_options(const tgs_options_t* o, bool batch = false)
{
    Opts r;
    r.prune = g_prune.load(std::memory_order_relaxed);
    r.deterministic = deterministic_mode();
    r.fwd_group = g_fwd_group.load(std::memory_order_relaxed);
    r.sort_cap = g_sort_cap.load(std::memory_order_relaxed);
    r.tile_bound = t_tile_bound; r.heavy_bound = 0; r.mid_bound = 0;
    static const int env_light = [] { const char* e = getenv("TGS_LIGHT_TILES"); return e ? atoi(e) : -1; }();     // A/B knob, read once
    r.light = env_light >= 0 ? (env_light ? 1 : 0) : (batch ? TGS_LIGHT_TILES_DEFAULT : 0);
    if (!o) return r;
    const size_t n = o->struct_size;
#define TGS_HAS(f) (n >= offsetof(tgs_options_t, f) + sizeof(o->f))
    if (TGS_HAS(instance_pruning) && o->instance_pruning >= 0) r.prune = o->instance_pruning ? 1 : 0;
    if (TGS_HAS(deterministic) && o->deterministic >= 0) r.deterministic = o->deterministic != 0;
    if (TGS_HAS(forward_group) && o->forward_group > 0) r.fwd_group = o->forward_group > BATCH_VIEWS ? BATCH_VIEWS : o->forward_group;
    if (TGS_HAS(sort_lds_cap) && o->sort_lds_cap >= 2 && o->sort_lds_cap <= SORT_LDS_CAP && !(o->sort_lds_cap & (o->sort_lds_cap - 1))) r.sort_cap = o->sort_lds_cap;
    if (TGS_HAS(tile_bound)) r.tile_bound = o->tile_bound > 0 ? o->tile_bound : 0;      // (explicit options: 0 really means none)
    if (TGS_HAS(heavy_bound) && o->heavy_bound > 0) r.heavy_bound = o->heavy_bound;
    if (TGS_HAS(mid_bound) && o->mid_bound > 0) r.mid_bound = o->mid_bound;
    if (TGS_HAS(light_tiles) && o->light_tiles >= 0) r.light = o->light_tiles ? 1 : 0;
#undef TGS_HAS
    return r;
}

// ---- optional per-stage timing (bench only): hipEvents recorded on the caller's stream, no sync ----
#include <mutex>
#include <vector>
namespace {
struct ProfRec { int stage; hipEvent_t e0, e1; };
std::mutex g_prof_mu;
bool g_prof_on = false;
size_t g_prof_cap = 0;
std::vector<ProfRec> g_prof;
hipEvent_t g_prof_open = nullptr;

unsigned g_prof_mask = ~0u;          // stages that get events (tgs_profile_stages)

void prof_begin_stage(hipStream_t st, int stage)
{
    if (!g_prof_on || !((g_prof_mask >> stage) & 1u)) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_on || g_prof.size() >= g_prof_cap) { g_prof_open = nullptr; return; }
    if (hipEventCreate(&g_prof_open) != hipSuccess) { g_prof_open = nullptr; return; }
    (void)hipEventRecord(g_prof_open, st);
}
void prof_end_stage(hipStream_t st, int stage)
{
    if (!g_prof_on || !((g_prof_mask >> stage) & 1u)) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_open) return;
    ProfRec r; r.stage = stage; r.e0 = g_prof_open; g_prof_open = nullptr;
    if (hipEventCreate(&r.e1) != hipSuccess) { (void)hipEventDestroy(r.e0); return; }
    (void)hipEventRecord(r.e1, st);
    g_prof.push_back(r);
}
}  // namespace

namespace tgs {
int set_error(int code, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}
int hip_status(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return TGS_OK;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return TGS_ERR_HIP;
}
}  // namespace tgs

static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
// an entry point that shares its implementation with others names itself in front of the message that implementation left
static int named(const char* fn, int r)
{
    if (r >= 0) return r;
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    return fail(r, "%s: %s", fn, msg);
}

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail(TGS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// One pipeline stage: profile events around `launch` on `st`, then the reference's CHECK_CUDA (auxiliary.h:166-173): in debug mode
// synchronise after every stage
template <class Launch>
static int stage(hipStream_t st, int id, const char* name, int debug, Launch&& launch)
{
    prof_begin_stage(st, id);
    launch();
    prof_end_stage(st, id);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && debug) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(TGS_ERR_HIP, "stage %s: %s", name, hipGetErrorString(e));
    return TGS_OK;
}

// ---- argument records: every extern "C" entry point packs its arguments into these ONCE (fields in the order of the C signatures);
// nothing below the entry points takes the long lists ----
struct GeomShape { size_t P; bool has_sh, has_sr; };      // what sizes the geometry buffer
struct Model {                  // the Gaussians: what every view of a call shares
    int P, D, M;
    const float *means3D, *shs, *colors_precomp, *opacities, *scales;
    float scale_modifier;
    const float *rotations, *cov3D_precomp;
    bool has_sh() const { return shs != nullptr; }
    bool has_sr() const { return scales != nullptr && rotations != nullptr; }
    GeomShape shape() const { return GeomShape{(size_t)P, has_sh(), has_sr()}; }
};

struct ViewArgs {               // one camera and its image; the one place that knows the tile grid
    const float* background;
    int width, height;
    const float *viewmatrix, *projmatrix, *campos;
    float tan_fovx, tan_fovy;
    uint32_t gx() const { return (uint32_t)((width + TILE - 1) / TILE); }
    uint32_t gy() const { return (uint32_t)((height + TILE - 1) / TILE); }
    size_t N() const { return (size_t)width * height; }
    size_t T() const { return (size_t)gx() * gy(); }
    CamParams cam(float scale_modifier) const
    {
        CamParams c;
        c.view = viewmatrix; c.proj = projmatrix; c.campos = campos;
        c.tan_fovx = tan_fovx; c.tan_fovy = tan_fovy;
        c.focal_y = height / (2.0f * tan_fovy);       // rasterizer_impl.cu:222-223
        c.focal_x = width / (2.0f * tan_fovx);
        c.scale_modifier = scale_modifier;
        c.W = width; c.H = height;
        c.gx = gx(); c.gy = gy();
        return c;
    }
};
static ViewArgs view_args(const tgs_view_t& v) { return ViewArgs{v.background, v.width, v.height, v.viewmatrix, v.projmatrix, v.campos, v.tan_fovx, v.tan_fovy}; }

static int frame_cam(CamParams& cam, const ViewArgs& v, float scale_modifier)
{
    cam = v.cam(scale_modifier);
    if (cam.gx > 65535u || cam.gy > 65535u) return fail(TGS_ERR_INVALID, "image too large");
    return TGS_OK;
}

struct FrameBuffers { GeomState g; ImgState s; BinState b; };      // the three state buffers of a frame, carved

// a frame whose buffers exist (backward, batch backward, tgs_state_field); a buffer the caller does not use may be NULL
static FrameBuffers carve_frame(const GeomShape& m, const ViewArgs& v, int64_t R, const void* geom, const void* binning, const void* img)
{
    FrameBuffers fb;
    geom_carve(fb.g, (char*)geom, m.P, m.has_sh, m.has_sr);
    img_carve(fb.s, (char*)img, v.N(), v.T());
    bin_carve(fb.b, (char*)binning, (size_t)R);
    return fb;
}

struct Alloc { tgs_alloc_fn fn; void* ctx; };

// the forward's frame: geometry and image are sized and requested first (in this order), the binning buffer once its size is known
static int alloc_geom_image(FrameBuffers& fb, const Alloc& a, const GeomShape& m, const ViewArgs& v)
{
    char* geom = (char*)a.fn(a.ctx, TGS_BUF_GEOM, geom_carve(fb.g, nullptr, m.P, m.has_sh, m.has_sr));
    char* img = (char*)a.fn(a.ctx, TGS_BUF_IMAGE, img_carve(fb.s, nullptr, v.N(), v.T()));
    if (!geom || !img) return fail(TGS_ERR_ALLOC, "state buffer allocation failed");
    fb = carve_frame(m, v, 0, geom, nullptr, img);
    return TGS_OK;
}
static int alloc_binning(FrameBuffers& fb, const Alloc& a, uint64_t R)
{
    char* bin = (char*)a.fn(a.ctx, TGS_BUF_BINNING, bin_carve(fb.b, nullptr, (size_t)R));
    if (!bin) return fail(TGS_ERR_ALLOC, "binning buffer allocation failed");
    bin_carve(fb.b, bin, (size_t)R);
    return TGS_OK;
}

// ---- the one model check and the one per-view check ----
// What the entry points ask of a model differs (and stays as it is): the single-view backward looks at neither D / M nor the model's
// pointers; only the forward refuses half a (scales, rotations) pair next to cov3D_precomp; the batch backward has no shared
// colors_precomp (shs == NULL there means per-view colours).
enum ModelUse { MODEL_FORWARD, MODEL_BACKWARD, MODEL_BATCH_BACKWARD };
static int check_model(const Model& m, ModelUse use)
{
    if (use != MODEL_BATCH_BACKWARD && m.has_sh() == (m.colors_precomp != nullptr)) return fail(TGS_ERR_INVALID, "provide exactly one of shs / colors_precomp");
    const bool half_pair = (m.scales == nullptr) != (m.rotations == nullptr);
    if (m.has_sr() == (m.cov3D_precomp != nullptr) || (use == MODEL_FORWARD && half_pair))
        return fail(TGS_ERR_INVALID, "provide exactly one of (scales, rotations) / cov3D_precomp");
    if (use == MODEL_BACKWARD) return TGS_OK;
    if (m.has_sh() && (m.D < 0 || m.D > 3 || m.M < (m.D + 1) * (m.D + 1)))
        return fail(TGS_ERR_INVALID, "SH degree %d needs M >= %d (M=%d)", m.D, (m.D + 1) * (m.D + 1), m.M);
    if (!m.means3D || (use == MODEL_FORWARD && !m.opacities)) return fail(TGS_ERR_INVALID, "NULL required pointer");
    return TGS_OK;
}

// A tgs_view_t carries the fields of three uses; each needs its own.  The per-pixel backward also serves tgs_backward_render, which has
// no view index to name: its two messages stay as they are.
enum ViewUse { VIEW_FORWARD, VIEW_RENDER_BWD, VIEW_BATCH_BWD };
static int check_view(const tgs_view_t& v, int k, ViewUse use, bool has_sh)
{
    const bool sizes = v.width > 0 && v.height > 0 && (use == VIEW_FORWARD || v.R >= 0);
    bool ptrs = v.binning_buffer && v.img_buffer;
    if (use == VIEW_RENDER_BWD) ptrs = ptrs && v.background && v.dL_dpix;
    else ptrs = ptrs && v.geom_buffer && v.viewmatrix && v.projmatrix && v.campos;
    if (use == VIEW_FORWARD) ptrs = ptrs && v.out_color && v.background;
    if (use == VIEW_BATCH_BWD) ptrs = ptrs && v.radii && v.dL_dmean2D && (has_sh || v.dL_dcolor);
    if (use == VIEW_RENDER_BWD) {
        if (!sizes) return fail(TGS_ERR_INVALID, "bad sizes");
        return ptrs ? TGS_OK : fail(TGS_ERR_INVALID, "NULL required pointer");
    }
    return sizes && ptrs ? TGS_OK : fail(TGS_ERR_INVALID, "view %d: bad sizes or NULL required pointer", k);
}

// ---- the bound rule, for both directions ----
// Sync-free grids cover `tiles` tiles (the caller's bound on the tiles with instances, or all T of them); k_scan rejects a frame with
// more.  The class bounds (tiles with >= 1024 / >= LIGHT_MAX instances) come with a tile bound below T only: only then does k_scan
// enforce them, and without that neither the forward nor the backward may size a grid by them.
struct Bounds { uint32_t tiles, heavy, mid; };
static Bounds all_tiles(size_t T) { return Bounds{(uint32_t)T, (uint32_t)T, (uint32_t)T}; }
static Bounds resolve_bounds(const Opts& o, size_t T)
{
    Bounds b = all_tiles(T);
    if (o.tile_bound > 0 && (uint64_t)o.tile_bound < (uint64_t)T) b.tiles = (uint32_t)o.tile_bound;
    const bool classes = b.tiles < T;
    b.heavy = (classes && o.heavy_bound > 0 && (uint64_t)o.heavy_bound < b.tiles) ? (uint32_t)o.heavy_bound : b.tiles;
    b.mid = (classes && o.mid_bound > 0 && (uint64_t)o.mid_bound < b.tiles) ? (uint32_t)o.mid_bound : b.tiles;
    return b;
}
// the bounds of a view of the *_views entry points travel in its tgs_view_t
static Opts view_options(Opts opt, const tgs_view_t& v)
{
    opt.tile_bound = v.tile_bound > 0 ? v.tile_bound : 0;
    opt.heavy_bound = v.heavy_bound > 0 ? v.heavy_bound : 0;
    opt.mid_bound = v.mid_bound > 0 ? v.mid_bound : 0;
    return opt;
}

// pinned Meta staging + event of the speculative forward: one per host thread AND device (an event belongs to the device that was
// current when it was created; a thread that renders on cuda:0 and then on cuda:1 gets a slot for each)
struct SpecSlot { Meta* meta; hipEvent_t ready; };
static SpecSlot* spec_slot()
{
    thread_local std::vector<SpecSlot> slots;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
    if ((size_t)dev >= slots.size()) slots.resize((size_t)dev + 1, SpecSlot{nullptr, nullptr});
    SpecSlot& slot = slots[(size_t)dev];
    if (!slot.meta) {
        if (hipHostMalloc((void**)&slot.meta, sizeof(Meta), hipHostMallocDefault) != hipSuccess) { slot.meta = nullptr; return nullptr; }
        if (hipEventCreateWithFlags(&slot.ready, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(slot.meta); slot.meta = nullptr; return nullptr; }
    }
    return &slot;
}

// tgs_set_render_streams: k_render_fwd of view k goes to render stream k mod n (behind an event on the view's own stream)
static thread_local std::vector<hipStream_t> t_render_streams;
static thread_local int64_t t_last_nonempty = -1;           // tgs_last_nonempty_tiles (legacy read-out; tgs_frame_info_t carries it explicitly)

// ---- the forward ----
// How one forward runs, beside the model and the view.  mode TGS_FWD_SYNC: the reference's protocol (read R back, then size the binning
// buffer).  TGS_FWD_ASYNC: sync-free -- the binning buffer is sized for r instances before anything runs and nothing is read back.
// TGS_FWD_SPECULATIVE: enqueued like the sync-free one against the guess r, then the host reads the frame's Meta and repeats the stages
// behind the scan if the guess was too small.
struct FwdCall {
    int mode; int64_t r; tgs_frame_info_t* info;
    Alloc alloc; hipStream_t st;
    int prefiltered; float* out_color; int* radii; int debug;
    // tgs_forward_views only: the pinned record k_scan writes the frame's Meta to as well; where k_render_fwd goes (nullptr: the frame's own
    // stream); whether the per-Gaussian stage of this view already ran with its group's
    Meta* host_meta; hipStream_t render_stream; bool preprocessed;
};
struct Forward {                // one forward in flight: what its phases share
    const Opts& opt; const FwdCall& c; const Model& m; const ViewArgs& v;
    CamParams cam; FrameBuffers fb; FwdIn in;
    uint32_t T() const { return (uint32_t)v.T(); }
};

static FwdIn fwd_in(const Model& m, const Opts& opt, int prefiltered)
{
    FwdIn in;
    memset(&in, 0, sizeof(in));
    in.P = m.P; in.D = m.D; in.M = m.M; in.means3D = m.means3D; in.shs = m.shs; in.colors_precomp = m.colors_precomp; in.opacities = m.opacities;
    in.scales = m.scales; in.rotations = m.rotations; in.cov3D_precomp = m.cov3D_precomp; in.prefiltered = prefiltered; in.prune = opt.prune;
    return in;
}

// rasterize_points.cu:81: nothing runs, the image keeps its zero fill (empty inputs have no pointers to check)
static int64_t forward_empty(const FwdCall& c, const ViewArgs& v)
{
    if (!c.out_color) return fail(TGS_ERR_INVALID, "NULL required pointer");
    HIP_TRY(hipMemsetAsync(c.out_color, 0, 3 * v.N() * sizeof(float), c.st));
    if (c.host_meta) memset(c.host_meta, 0, sizeof(Meta));   // (pinned host memory: no kernel of this frame writes it)
    if (c.info && c.mode != TGS_FWD_ASYNC) { c.info->num_rendered = 0; c.info->nonempty_tiles = 0; c.info->mid_tiles = 0; }
    if (c.mode != TGS_FWD_SYNC) {   // the caller still gets a (zeroed) Meta to query
        ImgState s0;
        char* ip = (char*)c.alloc.fn(c.alloc.ctx, TGS_BUF_IMAGE, img_carve(s0, nullptr, v.N(), v.T()));
        if (!ip) return fail(TGS_ERR_ALLOC, "state buffer allocation failed");
        HIP_TRY(hipMemsetAsync(ip, 0, 256, c.st));
    }
    return 0;
}

// validate, size and allocate geometry and image, fill the kernels' arguments.  Meta sits at the head of the image buffer;
// k_preprocess_fwd* clears it itself (block_sum_tiles: nothing else writes Meta before k_scan), everything else is written before it is
// read -- no memset launch in front of a frame
static int plan(Forward& f)
{
    if (int r = check_model(f.m, MODEL_FORWARD)) return r;
    if (!f.v.background || !f.v.viewmatrix || !f.v.projmatrix || !f.v.campos || !f.c.out_color) return fail(TGS_ERR_INVALID, "NULL required pointer");
    if (int r = frame_cam(f.cam, f.v, f.m.scale_modifier)) return r;
    if (int r = alloc_geom_image(f.fb, f.c.alloc, f.m.shape(), f.v)) return r;
    f.in = fwd_in(f.m, f.opt, f.c.prefiltered);
    f.in.background = f.v.background; f.in.out_color = f.c.out_color; f.in.radii = f.c.radii;
    return TGS_OK;
}

static int enqueue_preprocess(Forward& f)
{
    return stage(f.c.st, TGS_STAGE_PREPROCESS_FWD, "preprocess", f.c.debug, [&] { launch_preprocess_fwd(f.c.st, f.in, f.cam, f.fb.g, f.fb.s); });
}

// count and scan the tile instances; k_scan rejects a frame with more than `capacity` of them or more tiles than `b` allows, and writes
// the frame's Meta to `host_meta` as well when there is one
static int enqueue_scan(Forward& f, const Bounds& b, unsigned long long capacity, Meta* host_meta)
{
    return stage(f.c.st, TGS_STAGE_SCAN, "scan", f.c.debug, [&] {
        launch_bin_count(f.c.st, f.m.P, f.fb.g, f.fb.s, f.cam.gx, f.T());
        launch_scan(f.c.st, f.fb.g, f.fb.s, (uint32_t)n_blocks((size_t)f.m.P), f.T(), f.opt.sort_cap, capacity, b.tiles, b.heavy, b.mid, host_meta, f.opt.light);
    });
}

// what the host learns from a frame's Meta, once it has it; `flags`: the bits of Meta::error the caller is told about
static int read_meta(const FwdCall& c, const Meta& meta, uint32_t flags)
{
    if (meta.error & 1u) return fail(TGS_ERR_PREFILTERED, "Point is filtered although prefiltered is set. This shouldn't happen!");
    if (meta.R > 0x7fffffffull) return fail(TGS_ERR_TOO_MANY, "%llu tile instances exceed 2^31-1", (unsigned long long)meta.R);
    t_last_nonempty = (int64_t)meta.n_nonempty;
    if (c.info) { c.info->num_rendered = (int64_t)meta.R; c.info->nonempty_tiles = (int64_t)meta.n_nonempty; c.info->flags = (int32_t)(meta.error & flags); c.info->mid_tiles = (int32_t)meta.n_mid; }
    return TGS_OK;
}

// request the binning buffer for R instances, then scatter, tile sort and render.  `known`: the frame's Meta where the host has it (the
// kernels then size themselves by it).  render_stream: binning and compositing on different streams (tgs_set_render_streams)
static int enqueue_binning_and_render(Forward& f, uint64_t R, const Bounds& b, const Meta* known, hipStream_t render_stream)
{
    hipStream_t st = f.c.st;
    const int debug = f.c.debug;
    if (int r = alloc_binning(f.fb, f.c.alloc, R)) return r;
    if (R > 0) {
        if (int r = stage(st, TGS_STAGE_SCATTER, "scatter", debug, [&] { launch_scatter(st, f.m.P, f.fb.g, f.fb.s, f.fb.b, f.cam.gx, f.T()); })) return r;
        if (int r = stage(st, TGS_STAGE_TILE_SORT, "tile_sort", debug, [&] {
                launch_tile_sort(st, f.fb.g, f.fb.s, f.fb.b, f.cam.gx, f.T(), R, known, f.opt.sort_cap, b.tiles, b.heavy, b.mid); })) return r;
    }
    hipStream_t rst = st;
    if (render_stream && render_stream != st) {
        hipEvent_t binned;
        HIP_TRY(hipEventCreateWithFlags(&binned, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(binned, st));
        HIP_TRY(hipStreamWaitEvent(render_stream, binned, 0));
        (void)hipEventDestroy(binned);
        rst = render_stream;
    }
    // (the stage's events and its debug synchronisation stay on the frame's own stream)
    return stage(st, TGS_STAGE_RENDER_FWD, "render", debug, [&] {
        launch_render_fwd(rst, f.fb.s, f.fb.b, f.v.width, f.v.height, f.cam.gx, f.T(), known, f.v.background, f.c.out_color, b.tiles, b.mid, f.opt.light); });
}

static int64_t forward_impl(const Opts& opt, const FwdCall& c, const Model& m, const ViewArgs& v)
{
    const bool sync = c.mode == TGS_FWD_SYNC, spec = c.mode == TGS_FWD_SPECULATIVE;
    t_last_nonempty = -1;                                   // (known again once this call has read the frame's Meta)
    if (c.info) { c.info->num_rendered = -1; c.info->nonempty_tiles = -1; c.info->flags = 0; c.info->mid_tiles = -1; }
    if (!sync && c.r > 0x7fffffffll) return fail(TGS_ERR_INVALID, "r_capacity exceeds 2^31-1");
    g_err[0] = 0;
    if (!c.alloc.fn) return fail(TGS_ERR_INVALID, "alloc callback is NULL");
    if (m.P < 0 || v.width <= 0 || v.height <= 0) return fail(TGS_ERR_INVALID, "bad sizes P=%d W=%d H=%d", m.P, v.width, v.height);
    if (m.P == 0) return forward_empty(c, v);
    Forward f{opt, c, m, v};
    if (int r = plan(f)) return r;
    if (!c.preprocessed)
        if (int r = enqueue_preprocess(f)) return r;
    Meta meta;
    if (sync) {
        if (int r = enqueue_scan(f, all_tiles(v.T()), ~0ull, c.host_meta)) return r;
        // the one host synchronisation of the forward pass (rasterizer_impl.cu:280-281): R sizes the binning buffer
        HIP_TRY(hipMemcpyAsync(&meta, f.fb.s.meta, sizeof(Meta), hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        if (int r = read_meta(c, meta, ~0u)) return r;
        if (int r = enqueue_binning_and_render(f, meta.R, all_tiles(v.T()), &meta, c.render_stream)) return r;
        return (int64_t)meta.R;
    }
    const Bounds b = resolve_bounds(opt, v.T());
    if (!spec) {
        if (int r = enqueue_scan(f, b, (unsigned long long)c.r, c.host_meta)) return r;
        if (int r = enqueue_binning_and_render(f, (uint64_t)c.r, b, nullptr, c.render_stream)) return r;
        return c.r;
    }
    // speculative: k_scan itself writes Meta into the pinned host slot; the event marks its end, the remaining stages are enqueued
    // against the guessed capacity without waiting, and only then the host waits for the event -- the GPU never idles behind the
    // read-back, and no copy sits in the stream
    SpecSlot* slot = spec_slot();
    if (!slot) return fail(TGS_ERR_HIP, "pinned staging for the speculative forward could not be allocated");
    if (int r = enqueue_scan(f, b, (unsigned long long)c.r, slot->meta)) return r;
    HIP_TRY(hipEventRecord(slot->ready, c.st));
    if (int r = enqueue_binning_and_render(f, (uint64_t)c.r, b, nullptr, nullptr)) return r;
    HIP_TRY(hipEventSynchronize(slot->ready));
    meta = *slot->meta;
    if (int r = read_meta(c, meta, ~META_ERR_CAPACITY)) return r;
    if (!(meta.error & META_ERR_CAPACITY) && meta.pad[0] == 0u) return c.r;      // (pad[0]: more tiles with instances than the caller's bound, k_scan)
    // the guess was too small: every kernel behind the scan returned at once; clear the flag and run those stages again with the exact
    // sizes, as the synchronous forward does
    HIP_TRY(hipMemsetAsync(&f.fb.s.meta->error, 0, sizeof(uint32_t), c.st));
    if (int r = enqueue_binning_and_render(f, meta.R, all_tiles(v.T()), &meta, nullptr)) return r;
    return (int64_t)meta.R;
}

// ---- the backward ----
// the frame a backward differentiates and where its gradients go
struct BwdArgs {
    int64_t R; const int* radii; const void *geom_buffer, *binning_buffer, *img_buffer; const float* dL_dpix;
    float *dL_dmean2D, *dL_dconic, *dL_dopacity, *dL_dcolor, *dL_dmean3D, *dL_dcov3D, *dL_dsh, *dL_dscale, *dL_drot;
    const float* dL_dalpha = nullptr;       // upstream gradient of the accumulated alpha, [H * W] (tgs_backward_alpha_opt; NULL: none)
    const float* dL_ddepth = nullptr;       // upstream gradient of the expected depth, [H * W] (tgs_backward_depth_opt; NULL: none, and no depth kernel runs)
    float* dz_scratch = nullptr;            // with dL_ddepth: R floats of the caller's, one per instance (the slab row has no free float for dz)
    // tgs_backward_features_opt: upstream gradient of the feature map, [C * H * W] (NULL: none, and no feature kernel runs); with it the
    // features [P * C], R * C floats of the caller's and the output dL_dfeatures [P * C]
    int C = 0; const float* features = nullptr; const float* dL_dfeat_map = nullptr; float* feat_scratch = nullptr; float* dL_dfeatures = nullptr;
};

static BwdIn bwd_in(const Model& m)
{
    BwdIn in;
    memset(&in, 0, sizeof(in));
    in.P = m.P; in.D = m.D; in.M = m.M; in.means3D = m.means3D; in.shs = m.shs; in.colors_precomp = m.colors_precomp; in.scales = m.scales;
    in.rotations = m.rotations; in.cov3D_precomp = m.cov3D_precomp;
    return in;
}

// the per-pixel half of a frame's backward; the tile partials stay in the binning buffer
static int enqueue_render_bwd(const Opts& opt, hipStream_t st, int debug, const FrameBuffers& fb, const ViewArgs& v, int64_t R, const float* dL_dpix,
                              const float* dL_dalpha = nullptr, const float* dL_ddepth = nullptr, float* dz_scratch = nullptr, const BwdArgs* feat = nullptr, int P = 0)
{
    if (R <= 0) return TGS_OK;
    const Bounds b = resolve_bounds(opt, v.T());
    return stage(st, TGS_STAGE_RENDER_BWD, "render_bwd", debug, [&] {
        launch_render_bwd(st, fb.s, fb.b, v.width, v.height, v.gx(), b.tiles, v.background, dL_dpix, dL_dalpha, opt.deterministic, b.mid, opt.light, (uint32_t)v.T());
        // the depth's shares are ADDED to the slab rows the launch above has written (same stream: ordered behind it)
        if (dL_ddepth) launch_depth_bwd(st, fb.s, fb.b, v.width, v.height, v.gx(), b.tiles, (size_t)R, dL_ddepth, dz_scratch);
        // so are the feature channels' (a group of 8 channels per launch, each adding its share)
        if (feat && feat->dL_dfeat_map)
            launch_feat_bwd(st, fb.s, fb.b, v.width, v.height, v.gx(), b.tiles, (size_t)R, P, feat->C, feat->features, feat->dL_dfeat_map, feat->feat_scratch); });
}

// strict: tgs_backward / tgs_backward_accumulate as the reference's Rasterizer::backward declares them (every output required);
// tgs_backward_opt: the outputs its caller discards may be NULL (dL_dconic; dL_dcolor with shs; dL_dcov3D with scales + rotations)
static int backward_impl(bool strict, const Opts& opt, int accumulate, hipStream_t st, int debug, const Model& m, const ViewArgs& v, const BwdArgs& a)
{
    g_err[0] = 0;
    if (m.P == 0) return TGS_OK;
    if (m.P < 0 || a.R < 0 || v.width <= 0 || v.height <= 0) return fail(TGS_ERR_INVALID, "bad sizes");
    if (int r = check_model(m, MODEL_BACKWARD)) return r;
    if (!a.geom_buffer || !a.binning_buffer || !a.img_buffer || !a.radii || !a.dL_dpix || !a.dL_dmean2D || !a.dL_dopacity || !a.dL_dmean3D ||
        (m.has_sh() && !a.dL_dsh) || (!m.has_sh() && !a.dL_dcolor) || (!m.has_sr() && !a.dL_dcov3D) ||
        (strict && (!a.dL_dconic || (!accumulate && (!a.dL_dcolor || !a.dL_dcov3D)))) || (a.dL_ddepth && !a.dz_scratch) || (a.dL_ddepth && !v.viewmatrix) ||
        (a.dL_dfeat_map && (!a.features || !a.feat_scratch || !a.dL_dfeatures)))
        return fail(TGS_ERR_INVALID, "NULL required pointer");
    if (a.dL_dfeat_map && (a.C < 1 || a.C > TGS_FEATURE_MAX_CHANNELS)) return fail(TGS_ERR_INVALID, "bad channel count C=%d (1 .. %d)", a.C, TGS_FEATURE_MAX_CHANNELS);
    const CamParams cam = v.cam(m.scale_modifier);
    const FrameBuffers fb = carve_frame(m.shape(), v, a.R, a.geom_buffer, a.binning_buffer, a.img_buffer);

    BwdIn in = bwd_in(m);
    in.background = v.background; in.radii = a.radii; in.dL_dpix = a.dL_dpix;
    in.dL_dmean2D = a.dL_dmean2D; in.dL_dconic = a.dL_dconic; in.dL_dopacity = a.dL_dopacity; in.dL_dcolor = a.dL_dcolor;
    in.dL_dmean3D = a.dL_dmean3D; in.dL_dcov3D = a.dL_dcov3D; in.dL_dsh = a.dL_dsh; in.dL_dscale = a.dL_dscale; in.dL_drot = a.dL_drot;
    in.accumulate = accumulate;
    in.meta = fb.s.meta;

    if (int r = enqueue_render_bwd(opt, st, debug, fb, v, a.R, a.dL_dpix, a.dL_dalpha, a.dL_ddepth, a.dz_scratch, &a, m.P)) return r;
    return stage(st, TGS_STAGE_PREPROCESS_BWD, "preprocess_bwd", debug, [&] {
        launch_preprocess_bwd(st, in, cam, fb.g, fb.b);
        // dz . (third row of the view transform) is added behind the per-Gaussian pass: it holds for `accumulate` as well
        if (a.dL_ddepth && a.R > 0) launch_depth_bwd_gauss(st, m.P, fb.s.meta, a.radii, fb.g, v.viewmatrix, a.dz_scratch, a.dL_dmean3D);
        // the feature rows of every Gaussian (a frame without instances: zero rows, the scratch is not read)
        if (a.dL_dfeat_map) launch_feat_bwd_gauss(st, m.P, a.C, fb.s.meta, a.radii, fb.g, a.feat_scratch, a.dL_dfeatures, accumulate); });
}

// tgs_backward_render[_views]: the view's own fields (tgs_backward_render packs its arguments into one)
// feat (tgs_backward_render_views_features_opt): C, features, dL_dfeat_map and feat_scratch of the view, the only fields looked at
static int backward_render_impl(const Opts& opt, hipStream_t st, int P, const tgs_view_t& w, const float* dL_dalpha = nullptr, const float* dL_ddepth = nullptr,
                                float* dz_scratch = nullptr, const BwdArgs* feat = nullptr)
{
    g_err[0] = 0;
    if (P == 0) return TGS_OK;
    if (P < 0) return fail(TGS_ERR_INVALID, "bad sizes");
    if (int r = check_view(w, 0, VIEW_RENDER_BWD, false)) return r;
    if (dL_ddepth && !dz_scratch) return fail(TGS_ERR_INVALID, "NULL required pointer");
    const ViewArgs v = view_args(w);
    return enqueue_render_bwd(opt, st, 0, carve_frame(GeomShape{(size_t)P, false, false}, v, w.R, nullptr, w.binning_buffer, w.img_buffer), v, w.R, w.dL_dpix, dL_dalpha,
                              dL_ddepth, dz_scratch, feat, P);
}

// Element k of a caller's array of tgs_view_extras_t / tgs_view_features_t: the array's struct_size (its first element's) is the stride and the
// valid prefix of every element; fields beyond the caller's build read as NULL / 0.  `min_size`: the end of the first field a caller must
// have, `min_what` names it.  base == NULL: no view has any, every field reads as NULL.
template <class T>
static int read_element(const T* base, int k, T& out, const char* type, size_t min_size, const char* min_what)
{
    memset(&out, 0, sizeof(out));
    if (!base) return TGS_OK;
    const size_t stride = base->struct_size;
    if (stride < min_size) return fail(TGS_ERR_INVALID, "%s: struct_size %zu is smaller than %s", type, stride, min_what);
    memcpy(&out, (const char*)base + (size_t)k * stride, stride < sizeof(out) ? stride : sizeof(out));
    if (out.struct_size != stride) return fail(TGS_ERR_INVALID, "view %d: %s.struct_size %u differs from the array's %zu", k, type, out.struct_size, stride);
    return TGS_OK;
}
static int read_extras(const tgs_view_extras_t* base, int k, tgs_view_extras_t& out)
{
    if (int r = read_element(base, k, out, "tgs_view_extras_t", offsetof(tgs_view_extras_t, out_alpha) + sizeof(out.out_alpha), "the first pointer field")) return r;
    if (out.dL_ddepth && !out.dz_scratch) return fail(TGS_ERR_INVALID, "view %d: dL_ddepth without dz_scratch", k);
    return TGS_OK;
}
// an element TAKES PART when it has features, out_features or dL_dfeature_map
static bool feats_part(const tgs_view_features_t& x) { return x.features || x.out_features || x.dL_dfeature_map; }
static int read_feats(const tgs_view_features_t* base, int k, tgs_view_features_t& out)
{
    if (int r = read_element(base, k, out, "tgs_view_features_t", offsetof(tgs_view_features_t, features) + sizeof(out.features), "the end of the features field")) return r;
    if (!feats_part(out)) return TGS_OK;
    if (out.C < 1 || out.C > TGS_FEATURE_MAX_CHANNELS) return fail(TGS_ERR_INVALID, "view %d: bad channel count C=%d (1 .. %d)", k, out.C, TGS_FEATURE_MAX_CHANNELS);
    if (!out.features) return fail(TGS_ERR_INVALID, "view %d: out_features / dL_dfeature_map without features", k);
    if (out.dL_dfeature_map && !out.feature_scratch) return fail(TGS_ERR_INVALID, "view %d: dL_dfeature_map without feature_scratch", k);
    return TGS_OK;
}
// an element's three maps come together or not at all; the gradient needs the position map the forward left and a scratch
static int read_median(const tgs_view_median_t* base, int k, tgs_view_median_t& out)
{
    if (int r = read_element(base, k, out, "tgs_view_median_t", offsetof(tgs_view_median_t, out_depth) + sizeof(out.out_depth), "the first pointer field")) return r;
    const int outs = (out.out_depth != nullptr) + (out.out_index != nullptr) + (out.out_pos != nullptr);
    if (outs != 0 && outs != 3) return fail(TGS_ERR_INVALID, "view %d: out_depth, out_index and out_pos come together or not at all", k);
    if (out.dL_dmedian_depth && !out.dz_scratch) return fail(TGS_ERR_INVALID, "view %d: dL_dmedian_depth without dz_scratch", k);
    if (out.dL_dmedian_depth && !out.out_pos) return fail(TGS_ERR_INVALID, "view %d: dL_dmedian_depth without out_pos (the map tgs_median_views wrote)", k);
    return TGS_OK;
}

// The arguments the entry points with a tgs_view_extras_t, a tgs_view_features_t and / or a tgs_view_median_t array share, checked before
// anything is enqueued: the sizes and the views, then every element of the extras, of the feats, of the med (an array the call does not
// take: NULL).
// -> C of the elements that take part (the features are the model's: C and the pointer are the same in all of them; 0: none takes part)
static int check_views_call(int P, int n_views, const tgs_view_t* views, const tgs_view_extras_t* extras, const tgs_view_features_t* feats, int& C,
                            const tgs_view_median_t* med = nullptr)
{
    g_err[0] = 0;
    C = 0;
    if (P < 0 || n_views < 0) return fail(TGS_ERR_INVALID, "bad sizes P=%d n_views=%d", P, n_views);
    if (n_views > 0 && !views) return fail(TGS_ERR_INVALID, "NULL required pointer (views)");
    tgs_view_extras_t x;
    for (int k = 0; k < n_views && extras; k++)
        if (int r = read_extras(extras, k, x)) return r;
    tgs_view_features_t c;
    const float* features = nullptr;
    for (int k = 0; k < n_views && feats; k++) {
        if (int r = read_feats(feats, k, c)) return r;
        if (!feats_part(c)) continue;
        if (C == 0) { C = c.C; features = c.features; }
        else if (c.C != C || c.features != features)
            return fail(TGS_ERR_INVALID, "view %d: C=%d / features differ from an earlier view's (C=%d): the features are the model's, one tensor for all views", k, c.C, C);
    }
    tgs_view_median_t m;
    for (int k = 0; k < n_views && med; k++)
        if (int r = read_median(med, k, m)) return r;
    return TGS_OK;
}
static int check_streams(void* const* streams, int n_streams, int n_views)
{
    if ((n_views > 0 && !streams) || n_streams <= 0) return fail(TGS_ERR_INVALID, "bad arguments (streams, n_streams=%d)", n_streams);
    return TGS_OK;
}

// The per-pixel backward of several views, view k on streams[k % n_streams]: tgs_backward_render_views_opt and, with the views' extras and
// feature elements (either array may be NULL: no view has any), its two extensions.  The arrays were checked by the caller.
static int backward_render_views(const tgs_options_t* o, void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views,
                                 const tgs_view_extras_t* extras, const tgs_view_features_t* feats)
{
    const Opts opt0 = resolve_options(o, true);
    for (int k = 0; k < n_views; k++) {
        tgs_view_extras_t x;
        tgs_view_features_t f;
        if (int r = read_extras(extras, k, x)) return r;
        if (int r = read_feats(feats, k, f)) return r;
        BwdArgs fa{};
        fa.C = f.C; fa.features = f.features; fa.dL_dfeat_map = f.dL_dfeature_map; fa.feat_scratch = f.feature_scratch;
        const int r = backward_render_impl(view_options(opt0, views[k]), (hipStream_t)streams[k % n_streams], P, views[k], x.dL_dalpha, x.dL_ddepth, x.dz_scratch,
                                           f.dL_dfeature_map ? &fa : nullptr);
        if (r < 0) return r;
    }
    return TGS_OK;
}

// tgs_backward_render_views_extras_opt / _features_opt, under their name `fn`: the arrays, then the streams, then the loop
static int backward_render_views_checked(const char* fn, const tgs_options_t* o, void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views,
                                         const tgs_view_extras_t* extras, const tgs_view_features_t* feats)
{
    int C;
    if (int r = check_views_call(P, n_views, views, extras, feats, C)) return named(fn, r);
    if (int r = check_streams(streams, n_streams, n_views)) return named(fn, r);
    return named(fn, backward_render_views(o, streams, n_streams, P, n_views, views, extras, feats));
}

// The Gaussians [first, first + count) of a per-Gaussian pass over a batch: whole blocks of PRE_BLOCK, or the model's last ones
static int check_gaussian_range(int P, int first, int count)
{
    if (first < 0 || count < 0 || first % PRE_BLOCK != 0 || (long long)first + count > P || ((first + count) % PRE_BLOCK != 0 && first + count != P))
        return fail(TGS_ERR_INVALID, "Gaussian range [%d, %d + %d) must start and end on multiples of %d (or end at P = %d)", first, first, count, PRE_BLOCK, P);
    return TGS_OK;
}

// ---- a finished frame, opened for reading (the extra outputs: depth, median, features; alpha and depth / features of a batch's views) ----
// The one place that knows what such a call asks of a frame: P, R >= 0 and an image; with P == 0 or R == 0 nothing was blended (an empty
// model writes no image state at all) and no buffer is looked at; otherwise the state buffers the call reads, and a tile grid that fits a
// launch.  The callers say it in their own words and order: open_frame for the one-view calls, outputs_views for view k of a batch.
struct Frame {
    ViewArgs v; FrameBuffers fb;
    bool sizes_ok, blended, buffers_ok, grid_ok;
};
static Frame frame_facts(int P, int width, int height, int64_t R, const void* geom, const void* binning, const void* img, bool image_only = false)
{
    Frame f{};
    f.v = ViewArgs{nullptr, width, height, nullptr, nullptr, nullptr, 0.f, 0.f};
    f.sizes_ok = P >= 0 && R >= 0 && width > 0 && height > 0;
    f.blended = P > 0 && R > 0;
    f.buffers_ok = img && (image_only || (geom && binning));
    f.grid_ok = f.sizes_ok && f.v.gx() <= 65535u && f.v.gy() <= 65535u;
    if (f.sizes_ok && f.blended && f.buffers_ok && f.grid_ok) f.fb = carve_frame(GeomShape{(size_t)P, false, false}, f.v, R, geom, binning, img);
    return f;
}
// one view's call `fn`; own_ptrs: the call's own pointers are all there.  -> 1: launch; 0: nothing was blended and nothing is launched (the
// caller's fill stands); < 0: the error
static int open_frame(Frame& f, const char* fn, int P, int width, int height, int64_t R, const void* geom, const void* binning, const void* img, bool own_ptrs)
{
    g_err[0] = 0;
    f = frame_facts(P, width, height, R, geom, binning, img);
    if (!f.sizes_ok) return fail(TGS_ERR_INVALID, "%s: bad sizes P=%d W=%d H=%d R=%lld", fn, P, width, height, (long long)R);
    if (!f.blended) return 0;
    if (!f.buffers_ok || !own_ptrs) return fail(TGS_ERR_INVALID, "%s: NULL required pointer", fn);
    if (!f.grid_ok) return fail(TGS_ERR_INVALID, "%s: image too large", fn);
    return 1;
}
// The extra outputs of several views of a finished tgs_forward_views call, view k on streams[k % n_streams]: alpha and depth (tgs_outputs_views)
// the feature map (tgs_features_views) and the median maps (tgs_median_views), under their name `fn` -- any array may be NULL: no view has
// any.  A view in which nothing was blended has its outputs zero-filled (the median's index map: -1).
static int outputs_views(const char* fn, void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views, const tgs_view_extras_t* extras,
                         const tgs_view_features_t* feats, const tgs_view_median_t* med = nullptr)
{
    int C;
    if (int r = check_views_call(P, n_views, views, extras, feats, C, med)) return named(fn, r);
    if (int r = check_streams(streams, n_streams, n_views)) return named(fn, r);
    for (int k = 0; k < n_views; k++) {
        tgs_view_extras_t x;
        tgs_view_features_t c;
        if (int r = read_extras(extras, k, x)) return named(fn, r);
        tgs_view_median_t m;
        if (int r = read_feats(feats, k, c)) return named(fn, r);
        if (int r = read_median(med, k, m)) return named(fn, r);
        if (!x.out_alpha && !x.out_depth && !c.out_features && !m.out_depth) continue;
        const tgs_view_t& w = views[k];
        hipStream_t st = (hipStream_t)streams[k % n_streams];
        const Frame f = frame_facts(P, w.width, w.height, w.R, w.geom_buffer, w.binning_buffer, w.img_buffer, !x.out_depth && !c.out_features && !m.out_depth);
        if (!f.sizes_ok) return fail(TGS_ERR_INVALID, "%s: view %d: bad sizes", fn, k);
        if (!f.grid_ok) return fail(TGS_ERR_INVALID, "%s: view %d: image too large", fn, k);
        const size_t N = f.v.N();
        if (!f.blended) {
            if (x.out_alpha) HIP_TRY(hipMemsetAsync(x.out_alpha, 0, N * sizeof(float), st));
            if (x.out_depth) HIP_TRY(hipMemsetAsync(x.out_depth, 0, N * sizeof(float), st));
            if (c.out_features) HIP_TRY(hipMemsetAsync(c.out_features, 0, (size_t)c.C * N * sizeof(float), st));
            if (m.out_depth) {
                HIP_TRY(hipMemsetAsync(m.out_depth, 0, N * sizeof(float), st));
                HIP_TRY(hipMemsetAsync(m.out_index, 0xff, N * sizeof(int32_t), st));
                HIP_TRY(hipMemsetAsync(m.out_pos, 0, N * sizeof(int32_t), st));
            }
            continue;
        }
        if (!f.buffers_ok) return fail(TGS_ERR_INVALID, "%s: view %d: NULL required pointer", fn, k);
        if (x.out_alpha) launch_alpha(st, f.fb.s, N, x.out_alpha);
        if (x.out_depth) launch_depth_fwd(st, f.fb.s, f.fb.b, w.width, w.height, f.v.gx(), (uint32_t)f.v.T(), x.out_depth);
        if (c.out_features) launch_feat_fwd(st, f.fb.s, f.fb.b, w.width, w.height, f.v.gx(), (uint32_t)f.v.T(), P, c.C, c.features, c.out_features);   // (zero-fills the map first)
        if (m.out_depth) launch_median_fwd(st, f.fb.s, f.fb.b, w.width, w.height, f.v.gx(), (uint32_t)f.v.T(), m.out_depth, m.out_index, m.out_pos);   // (fills 0 / -1 / 0 first)
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(TGS_ERR_HIP, "%s: view %d: %s", fn, k, hipGetErrorString(e));
    }
    return TGS_OK;
}

// The z-path of a gradient on view-space depths for all views in one pass over Gaussians [first, first + count): the body of
// tgs_backward_batch_depth_range and tgs_backward_batch_median_range, under their name `fn`.  rows_of(k, rows): the dz rows of view k (one float
// per instance slot), NULL: the view takes no part.  The arrays were checked by the caller.  One launch per BATCH_VIEWS views that take part.
template <class RowsOf>
static int z_path_range(const char* fn, hipStream_t st, int P, int n_views, const tgs_view_t* views, float* dL_dmean3D, int first, int count, RowsOf&& rows_of)
{
    if (P == 0 || n_views == 0 || count == 0) return TGS_OK;
    if (int r = check_gaussian_range(P, first, count)) return named(fn, r);
    DepthViews dv;
    memset(&dv, 0, sizeof(dv));
    auto flush = [&]() -> int {
        if (dv.n == 0) return TGS_OK;
        const int r = stage(st, TGS_STAGE_PREPROCESS_BWD, "depth_bwd_gauss_views", 0, [&] { launch_depth_bwd_gauss_views(st, first, count, dv, dL_dmean3D); });
        dv.n = 0;
        return r;
    };
    for (int k = 0; k < n_views; k++) {
        const float* rows = nullptr;
        if (int r = rows_of(k, rows)) return named(fn, r);
        const tgs_view_t& w = views[k];
        if (!rows || w.R <= 0) continue;                    // (R == 0: the per-pixel backward launched nothing and the scratch was not filled)
        if (!dL_dmean3D || !w.geom_buffer || !w.img_buffer || !w.radii || !w.viewmatrix || w.width <= 0 || w.height <= 0)
            return fail(TGS_ERR_INVALID, "%s: view %d: bad sizes or NULL required pointer", fn, k);
        const FrameBuffers fb = carve_frame(GeomShape{(size_t)P, false, false}, view_args(w), w.R, w.geom_buffer, nullptr, w.img_buffer);
        DepthView& d = dv.v[dv.n++];
        d.meta = fb.s.meta; d.radii = w.radii; d.tiles_touched = fb.g.tiles_touched; d.offsets = fb.g.offsets; d.dz_rows = rows; d.view = w.viewmatrix;
        if (dv.n == BATCH_VIEWS)
            if (int r = flush()) return named(fn, r);
    }
    return named(fn, flush());
}

// the shared per-Gaussian stage of a group of views of tgs_forward_views: one launch on the group's first stream
static int enqueue_group_preprocess(const Opts& opt, hipStream_t st, const Model& m, int prefiltered, const tgs_view_t* views, int v0, int nv)
{
    const FwdIn in = fwd_in(m, opt, prefiltered);
    FwdViews fv;
    memset(&fv, 0, sizeof(fv));
    fv.n = nv;
    for (int k = 0; k < nv; k++) {
        const tgs_view_t& w = views[v0 + k];
        const ViewArgs v = view_args(w);
        FwdView& o = fv.v[k];
        if (int r = frame_cam(o.cam, v, m.scale_modifier)) return r;
        if (geom_carve(o.g, nullptr, (size_t)m.P, m.has_sh(), m.has_sr()) > w.geom_bytes || img_carve(o.s, nullptr, v.N(), v.T()) > w.img_bytes)
            return fail(TGS_ERR_ALLOC, "view %d: state buffers smaller than tgs_state_sizes()", v0 + k);
        const FrameBuffers fb = carve_frame(m.shape(), v, 0, w.geom_buffer, nullptr, w.img_buffer);
        o.g = fb.g; o.s = fb.s;
        o.radii = w.radii_out;
    }
    return stage(st, TGS_STAGE_PREPROCESS_FWD, "preprocess_batch", 0, [&] { launch_preprocess_fwd_batch(st, in, fv); });
}

// allocation "callback" of the *_views entry points: hands out the caller's preset buffers
static void* alloc_preset(void* ctx, int which, size_t bytes)
{
    const tgs_view_t* v = (const tgs_view_t*)ctx;
    if (which == TGS_BUF_GEOM) return bytes <= v->geom_bytes ? const_cast<void*>(v->geom_buffer) : nullptr;
    if (which == TGS_BUF_BINNING) return bytes <= v->binning_bytes ? const_cast<void*>(v->binning_buffer) : nullptr;
    if (which == TGS_BUF_IMAGE) return bytes <= v->img_bytes ? const_cast<void*>(v->img_buffer) : nullptr;
    return nullptr;
}

extern "C" {

int tgs_abi_version(void) { return TGS_ABI_VERSION; }

void tgs_set_instance_pruning(int on) { g_prune.store(on ? 1 : 0, std::memory_order_relaxed); }

void tgs_set_forward_group(int views_per_launch)
{
    g_fwd_group.store(views_per_launch < 1 ? 1 : (views_per_launch > BATCH_VIEWS ? BATCH_VIEWS : views_per_launch), std::memory_order_relaxed);
}

int tgs_set_sort_lds_cap(unsigned cap)
{
    if (cap < 2 || cap > SORT_LDS_CAP || (cap & (cap - 1))) return fail(TGS_ERR_INVALID, "sort cap must be a power of two in [2, %u]", SORT_LDS_CAP);
    g_sort_cap.store(cap, std::memory_order_relaxed);
    return TGS_OK;
}

void tgs_set_deterministic(int on) { g_deterministic.store(on < 0 ? -1 : (on ? 1 : 0), std::memory_order_relaxed); }

int tgs_selftest_reduce36(void* stream, const float* in, float* out)
{
    launch_selftest_reduce36((hipStream_t)stream, in, out);
    return hipGetLastError() == hipSuccess ? TGS_OK : TGS_ERR_HIP;
}

int tgs_profile_begin(int max_records)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof_on) return TGS_ERR_INVALID;
    g_prof.clear();
    g_prof_cap = max_records > 0 ? (size_t)max_records : 0;
    g_prof.reserve(g_prof_cap);
    g_prof_open = nullptr;
    g_prof_on = true;
    return TGS_OK;
}

void tgs_profile_stages(unsigned mask)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_mask = mask;
}

int tgs_profile_end(double* ms_sum, int64_t* counts)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_on) return TGS_ERR_INVALID;
    g_prof_on = false;
    for (int i = 0; i < TGS_STAGE_COUNT; i++) { ms_sum[i] = 0.0; counts[i] = 0; }
    for (ProfRec& r : g_prof) {
        float ms = 0.f;
        if (hipEventSynchronize(r.e1) == hipSuccess && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess &&
            r.stage >= 0 && r.stage < TGS_STAGE_COUNT) { ms_sum[r.stage] += ms; counts[r.stage]++; }
        (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    }
    g_prof.clear();
    return TGS_OK;
}
const char* tgs_last_error(void) { return g_err; }

int64_t tgs_forward(tgs_alloc_fn alloc, void* alloc_ctx, void* stream, int P, int D, int M, const float* background, int width,
                    int height, const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                    const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                    int prefiltered, float* out_color, int* radii, int debug)
{
    return tgs_forward_opt(nullptr, TGS_FWD_SYNC, 0, nullptr, alloc, alloc_ctx, stream, P, D, M, background, width, height, means3D, shs, colors_precomp, opacities,
                           scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, out_color, radii, debug);
}

int64_t tgs_forward_opt(const tgs_options_t* o, int mode, int64_t r, tgs_frame_info_t* info, tgs_alloc_fn alloc, void* alloc_ctx, void* stream, int P, int D, int M,
                        const float* background, int width, int height, const float* means3D, const float* shs, const float* colors_precomp,
                        const float* opacities, const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                        const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                        float* out_color, int* radii, int debug)
{
    const Opts opt = resolve_options(o);
    if (mode != TGS_FWD_SYNC && mode != TGS_FWD_ASYNC && mode != TGS_FWD_SPECULATIVE) return fail(TGS_ERR_INVALID, "tgs_forward_opt: unknown mode %d", mode);
    if (mode != TGS_FWD_SYNC && r < 0) return fail(TGS_ERR_INVALID, "r_capacity / r_guess must be >= 0");
    const FwdCall c{mode, r, info, {alloc, alloc_ctx}, (hipStream_t)stream, prefiltered, out_color, radii, debug, nullptr, nullptr, false};
    return forward_impl(opt, c, Model{P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp},
                        ViewArgs{background, width, height, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy});
}

int64_t tgs_forward_async(int64_t r_capacity, tgs_alloc_fn alloc, void* alloc_ctx, void* stream, int P, int D, int M, const float* background,
                          int width, int height, const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                          const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                          const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                          int prefiltered, float* out_color, int* radii, int debug)
{
    if (r_capacity < 0) return fail(TGS_ERR_INVALID, "r_capacity must be >= 0");
    return tgs_forward_opt(nullptr, TGS_FWD_ASYNC, r_capacity, nullptr, alloc, alloc_ctx, stream, P, D, M, background, width, height, means3D, shs, colors_precomp, opacities,
                           scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, out_color, radii, debug);
}

int64_t tgs_forward_speculative(int64_t r_guess, int64_t* num_rendered, tgs_alloc_fn alloc, void* alloc_ctx, void* stream, int P, int D, int M,
                                const float* background, int width, int height, const float* means3D, const float* shs, const float* colors_precomp,
                                const float* opacities, const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                int prefiltered, float* out_color, int* radii, int debug)
{
    if (r_guess < 0 || !num_rendered) return fail(TGS_ERR_INVALID, "r_guess must be >= 0 and num_rendered non-NULL");
    *num_rendered = 0;
    tgs_frame_info_t info;
    const int64_t r = tgs_forward_opt(nullptr, TGS_FWD_SPECULATIVE, r_guess, &info, alloc, alloc_ctx, stream, P, D, M, background, width, height, means3D, shs, colors_precomp,
                                      opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, out_color,
                                      radii, debug);
    if (r >= 0 && info.num_rendered >= 0) *num_rendered = info.num_rendered;
    return r;
}

int tgs_frame_status(void* stream, const void* img_buffer, int64_t* num_rendered, int* flags)
{
    g_err[0] = 0;
    if (!img_buffer || !num_rendered || !flags) return fail(TGS_ERR_INVALID, "NULL required pointer");
    Meta meta;
    ImgState s;
    img_carve(s, (char*)img_buffer, 0, 0);                  // Meta is the first field of the image buffer
    HIP_TRY(hipMemcpyAsync(&meta, s.meta, sizeof(Meta), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *num_rendered = (int64_t)meta.R;
    *flags = (int)meta.error;
    if (meta.error & META_ERR_TILE_BOUND)
        return fail(TGS_ERR_INVALID, "a backward of this frame ran with a tile bound below its %u tiles with instances: gradients are incomplete", meta.n_nonempty);
    return TGS_OK;
}

// The six one-view backward entry points differ in the upstream gradients they take, in their name, and in how strict they are about
// outputs; the frame they differentiate and the gradients they write are one list, declared in include/tgs_raster.h six times (the compiler
// holds these definitions against it) and spelled here once: as parameters, and as the arguments handed on to the one packing.
#define TGS_BWD_FRAME_PARAMS                                                                                                               \
    void *stream, int P, int D, int M, int64_t R, const float *background, int width, int height, const float *means3D, const float *shs,  \
        const float *colors_precomp, const float *scales, float scale_modifier, const float *rotations, const float *cov3D_precomp,        \
        const float *viewmatrix, const float *projmatrix, const float *campos, float tan_fovx, float tan_fovy, const int *radii,           \
        const void *geom_buffer, const void *binning_buffer, const void *img_buffer, const float *dL_dpix
#define TGS_BWD_FRAME_ARGS                                                                                                                 \
    stream, P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp,         \
        viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, img_buffer, dL_dpix
#define TGS_BWD_GRAD_PARAMS                                                                                                                \
    float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh,         \
        float *dL_dscale, float *dL_drot, int debug
#define TGS_BWD_GRAD_ARGS dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, debug

// the upstream gradients beside dL_dpix, with what each needs (BwdArgs says what they are); an entry point leaves out what it does not take
struct Upstream {
    const float* dL_dalpha = nullptr;
    const float* dL_ddepth = nullptr; float* dz_scratch = nullptr;
    int C = 0; const float* features = nullptr; const float* dL_dfeature_map = nullptr; float* feature_scratch = nullptr; float* dL_dfeatures = nullptr;
};
static int backward_packed(bool strict, const Opts& opt, int accumulate, TGS_BWD_FRAME_PARAMS, const Upstream& u, TGS_BWD_GRAD_PARAMS)
{
    BwdArgs a{R, radii, geom_buffer, binning_buffer, img_buffer, dL_dpix, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, u.dL_dalpha};
    a.dL_ddepth = u.dL_ddepth; a.dz_scratch = u.dL_ddepth ? u.dz_scratch : nullptr;
    a.C = u.C; a.features = u.features; a.dL_dfeat_map = u.dL_dfeature_map; a.feat_scratch = u.feature_scratch; a.dL_dfeatures = u.dL_dfeatures;
    return backward_impl(strict, opt, accumulate ? 1 : 0, (hipStream_t)stream, debug,
                         Model{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp},
                         ViewArgs{background, width, height, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy}, a);
}

int tgs_backward(TGS_BWD_FRAME_PARAMS, TGS_BWD_GRAD_PARAMS)
{
    return backward_packed(true, resolve_options(nullptr), 0, TGS_BWD_FRAME_ARGS, Upstream{}, TGS_BWD_GRAD_ARGS);
}

int tgs_backward_accumulate(TGS_BWD_FRAME_PARAMS, TGS_BWD_GRAD_PARAMS)
{
    return backward_packed(true, resolve_options(nullptr), 1, TGS_BWD_FRAME_ARGS, Upstream{}, TGS_BWD_GRAD_ARGS);
}

int tgs_backward_opt(const tgs_options_t* o, int accumulate, TGS_BWD_FRAME_PARAMS, TGS_BWD_GRAD_PARAMS)
{
    return backward_packed(false, resolve_options(o), accumulate, TGS_BWD_FRAME_ARGS, Upstream{}, TGS_BWD_GRAD_ARGS);
}

int tgs_backward_alpha_opt(const tgs_options_t* o, int accumulate, TGS_BWD_FRAME_PARAMS, const float* dL_dalpha, TGS_BWD_GRAD_PARAMS)
{
    return named("tgs_backward_alpha_opt", backward_packed(false, resolve_options(o), accumulate, TGS_BWD_FRAME_ARGS, Upstream{dL_dalpha}, TGS_BWD_GRAD_ARGS));
}

int tgs_backward_depth_opt(const tgs_options_t* o, int accumulate, TGS_BWD_FRAME_PARAMS, const float* dL_dalpha, const float* dL_ddepth, float* dz_scratch,
                           TGS_BWD_GRAD_PARAMS)
{
    return named("tgs_backward_depth_opt",
                 backward_packed(false, resolve_options(o), accumulate, TGS_BWD_FRAME_ARGS, Upstream{dL_dalpha, dL_ddepth, dz_scratch}, TGS_BWD_GRAD_ARGS));
}

int tgs_backward_features_opt(const tgs_options_t* o, int accumulate, TGS_BWD_FRAME_PARAMS, const float* dL_dalpha, const float* dL_ddepth, float* dz_scratch,
                              int C, const float* features, const float* dL_dfeature_map, float* feature_scratch, float* dL_dfeatures, TGS_BWD_GRAD_PARAMS)
{
    // without a map this IS the depth call -- the other four arguments are not looked at -- and it says so in its errors
    return named(dL_dfeature_map ? "tgs_backward_features_opt" : "tgs_backward_depth_opt",
                 backward_packed(false, resolve_options(o), accumulate, TGS_BWD_FRAME_ARGS,
                                 Upstream{dL_dalpha, dL_ddepth, dz_scratch, C, features, dL_dfeature_map, feature_scratch, dL_dfeatures}, TGS_BWD_GRAD_ARGS));
}

void tgs_state_sizes(int P, int width, int height, int has_sh, int has_scale_rot, int64_t r_capacity, size_t sizes3[3])
{
    FrameBuffers fb;
    const ViewArgs v{nullptr, width, height, nullptr, nullptr, nullptr, 0.f, 0.f};
    sizes3[TGS_BUF_GEOM] = geom_carve(fb.g, nullptr, (size_t)(P > 0 ? P : 0), has_sh != 0, has_scale_rot != 0);
    sizes3[TGS_BUF_BINNING] = bin_carve(fb.b, nullptr, (size_t)(r_capacity > 0 ? r_capacity : 0));
    sizes3[TGS_BUF_IMAGE] = img_carve(fb.s, nullptr, v.N(), v.T());
}

void tgs_set_tile_bound(int64_t n) { t_tile_bound = n > 0 ? n : 0; }
int64_t tgs_last_nonempty_tiles(void) { return t_last_nonempty; }

int tgs_set_render_streams(void* const* streams, int n)
{
    t_render_streams.clear();
    for (int i = 0; i < n && streams; i++) t_render_streams.push_back((hipStream_t)streams[i]);
    return TGS_OK;
}

size_t tgs_sizeof_view(void) { return sizeof(tgs_view_t); }
size_t tgs_sizeof_options(void) { return sizeof(tgs_options_t); }

int tgs_forward_views(void* const* streams, int n_streams, int64_t r_capacity, int P, int D, int M, const float* means3D, const float* shs,
                      const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                      const float* cov3D_precomp, int prefiltered, int n_views, tgs_view_t* views)
{
    return tgs_forward_views_opt(nullptr, streams, n_streams, r_capacity, P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp,
                                 prefiltered, n_views, views);
}

int tgs_forward_views_opt(const tgs_options_t* o, void* const* streams, int n_streams, int64_t r_capacity, int P, int D, int M, const float* means3D, const float* shs,
                          const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                          const float* cov3D_precomp, int prefiltered, int n_views, tgs_view_t* views)
{
    const Opts opt0 = resolve_options(o, true);
    g_err[0] = 0;
    if (n_views == 0) return TGS_OK;
    if (!streams || n_streams <= 0 || n_views < 0 || !views || r_capacity < 0) return fail(TGS_ERR_INVALID, "bad arguments");
    const Model m{P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp};
    // Views per launch of the shared per-Gaussian stage (tgs_set_forward_group, TGS_FORWARD_GROUP; default 2).  More views per launch
    // read the SH rows -- more than half of what the stage reads -- fewer times: 51 us for one view, 78 / 125 / 218 us for 2 / 4 / 8.
    // But the views of a group start their remaining stages together, and with four streams that costs more than the bytes save
    // beyond pairs: 0.302 / 0.296 / 0.308 / 0.306 ms per frame for groups of 1 / 2 / 4 / 8 at config 3.  (With the counting atomics
    // in this stage, until round 2, the launch was bound by them and no grouping paid.)
    static const int env_group = [] { const char* e = getenv("TGS_FORWARD_GROUP"); return e ? atoi(e) : 0; }();   // tuning knob, read once
    int group = opt0.fwd_group;
    if (env_group > 0) group = env_group > BATCH_VIEWS ? BATCH_VIEWS : env_group;
    bool per_view_colors = false;
    for (int k = 0; k < n_views; k++) per_view_colors = per_view_colors || views[k].colors_precomp != nullptr;
    if (per_view_colors && shs) return fail(TGS_ERR_INVALID, "provide exactly one of shs / colors_precomp");
    // views that share the per-Gaussian stage: same colours, a model the forward accepts (any other takes the single-view route, whose
    // forward names the error)
    const bool batched = !per_view_colors && group > 1 && n_views > 1 && P > 0 && check_model(m, MODEL_FORWARD) == TGS_OK;
    for (int v0 = 0; v0 < n_views; v0 += group) {
        const int nv = n_views - v0 < group ? n_views - v0 : group;
        hipStream_t st0 = (hipStream_t)streams[v0 % n_streams];
        hipEvent_t pre_done = nullptr;
        for (int k = 0; k < nv; k++)
            if (int r = check_view(views[v0 + k], v0 + k, VIEW_FORWARD, false)) return r;
        if (batched) {
            if (int r = enqueue_group_preprocess(opt0, st0, m, prefiltered, views, v0, nv)) return r;
            if (n_streams > 1) {
                HIP_TRY(hipEventCreateWithFlags(&pre_done, hipEventDisableTiming));
                HIP_TRY(hipEventRecord(pre_done, st0));
            }
        }
        for (int k = 0; k < nv; k++) {
            tgs_view_t& v = views[v0 + k];
            hipStream_t st = (hipStream_t)streams[(v0 + k) % n_streams];
            if (pre_done && st != st0) HIP_TRY(hipStreamWaitEvent(st, pre_done, 0));
            hipStream_t render_stream = t_render_streams.empty() ? nullptr : t_render_streams[(size_t)(v0 + k) % t_render_streams.size()];
            Model mv = m;
            if (v.colors_precomp) mv.colors_precomp = v.colors_precomp;
            const FwdCall c{TGS_FWD_ASYNC, r_capacity, nullptr, {alloc_preset, &v}, st, prefiltered, v.out_color, v.radii_out, 0, (Meta*)v.host_meta, render_stream, batched};
            const int64_t r = forward_impl(view_options(opt0, v), c, mv, view_args(v));
            if (r < 0) { if (pre_done) (void)hipEventDestroy(pre_done); return (int)r; }
            v.R = r;
        }
        if (pre_done) (void)hipEventDestroy(pre_done);
    }
    return TGS_OK;
}

int tgs_backward_render_views(void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views)
{
    return tgs_backward_render_views_opt(nullptr, streams, n_streams, P, n_views, views);
}

int tgs_backward_render_views_opt(const tgs_options_t* o, void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views)
{
    if (n_views == 0) return TGS_OK;
    if (!streams || n_streams <= 0 || n_views < 0 || !views) return fail(TGS_ERR_INVALID, "bad arguments");
    return backward_render_views(o, streams, n_streams, P, n_views, views, nullptr, nullptr);
}

size_t tgs_sizeof_view_extras(void) { return sizeof(tgs_view_extras_t); }

int tgs_outputs_views(void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views, const tgs_view_extras_t* extras)
{
    return outputs_views("tgs_outputs_views", streams, n_streams, P, n_views, views, extras, nullptr);
}

int tgs_backward_render_views_extras_opt(const tgs_options_t* o, void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views,
                                         const tgs_view_extras_t* extras)
{
    return backward_render_views_checked("tgs_backward_render_views_extras_opt", o, streams, n_streams, P, n_views, views, extras, nullptr);
}

int tgs_backward_batch_depth_range(void* stream, int P, int n_views, const tgs_view_t* views, const tgs_view_extras_t* extras, float* dL_dmean3D, int first, int count)
{
    static const char* fn = "tgs_backward_batch_depth_range";
    int C;
    if (int r = check_views_call(P, n_views, views, extras, nullptr, C)) return named(fn, r);
    if (!extras) return TGS_OK;
    return z_path_range(fn, (hipStream_t)stream, P, n_views, views, dL_dmean3D, first, count, [&](int k, const float*& rows) -> int {
        tgs_view_extras_t x;
        if (int r = read_extras(extras, k, x)) return r;
        rows = x.dL_ddepth ? x.dz_scratch : nullptr;
        return TGS_OK;
    });
}

size_t tgs_sizeof_view_features(void) { return sizeof(tgs_view_features_t); }

int tgs_features_views(void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views, const tgs_view_features_t* feats)
{
    return outputs_views("tgs_features_views", streams, n_streams, P, n_views, views, nullptr, feats);
}

int tgs_backward_render_views_features_opt(const tgs_options_t* o, void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views,
                                           const tgs_view_extras_t* extras, const tgs_view_features_t* feats)
{
    return backward_render_views_checked("tgs_backward_render_views_features_opt", o, streams, n_streams, P, n_views, views, extras, feats);
}

int tgs_backward_batch_features_range(void* stream, int P, int n_views, const tgs_view_t* views, const tgs_view_features_t* feats, float* dL_dfeatures,
                                      int accumulate, int first, int count)
{
    static const char* fn = "tgs_backward_batch_features_range";
    hipStream_t st = (hipStream_t)stream;
    int C;
    if (int r = check_views_call(P, n_views, views, nullptr, feats, C)) return named(fn, r);
    if (P == 0 || n_views == 0 || count == 0 || !feats || C == 0) return TGS_OK;
    if (int r = check_gaussian_range(P, first, count)) return named(fn, r);
    if ((unsigned long long)count * (unsigned)((C + 3) / 4) > 0xffffff00ull) return fail(TGS_ERR_INVALID, "%s: range of %d Gaussians x %d channels is too large for one call", fn, count, C);
    // the views that take part: a gradient of the map, and instances (R == 0: the per-pixel backward launched nothing and the scratch was not filled)
    int n_part = 0;
    for (int k = 0; k < n_views; k++) {
        tgs_view_features_t x;
        if (int r = read_feats(feats, k, x)) return named(fn, r);
        const tgs_view_t& w = views[k];
        if (!x.dL_dfeature_map) continue;
        if (!dL_dfeatures) return fail(TGS_ERR_INVALID, "%s: view %d has dL_dfeature_map but dL_dfeatures is NULL", fn, k);
        if (w.R <= 0) continue;
        if (!w.geom_buffer || !w.img_buffer || !w.radii || w.width <= 0 || w.height <= 0) return fail(TGS_ERR_INVALID, "%s: view %d: bad sizes or NULL required pointer", fn, k);
        n_part++;
    }
    if (n_part == 0) {                                      // store: the range is defined all the same; accumulate: nothing to add
        if (!accumulate && dL_dfeatures) HIP_TRY(hipMemsetAsync(dL_dfeatures + (size_t)first * C, 0, (size_t)count * C * sizeof(float), st));
        return TGS_OK;
    }
    FeatViews fv;
    memset(&fv, 0, sizeof(fv));
    bool vec = C % 4 == 0 && (uintptr_t)dL_dfeatures % 16 == 0;
    int acc = accumulate ? 1 : 0;                           // the first launch of the call honours `accumulate`, the later ones add
    auto flush = [&]() -> int {
        if (fv.n == 0) return TGS_OK;
        const int r = stage(st, TGS_STAGE_PREPROCESS_BWD, "feat_bwd_gauss_views", 0, [&] { launch_feat_bwd_gauss_views(st, first, count, C, fv, dL_dfeatures, acc, vec); });
        fv.n = 0; acc = 1;
        vec = C % 4 == 0 && (uintptr_t)dL_dfeatures % 16 == 0;
        return r;
    };
    for (int k = 0; k < n_views; k++) {
        tgs_view_features_t x;
        if (int r = read_feats(feats, k, x)) return named(fn, r);
        const tgs_view_t& w = views[k];
        if (!x.dL_dfeature_map || w.R <= 0) continue;
        const FrameBuffers fb = carve_frame(GeomShape{(size_t)P, false, false}, view_args(w), w.R, w.geom_buffer, nullptr, w.img_buffer);
        FeatView& d = fv.v[fv.n++];
        d.meta = fb.s.meta; d.radii = w.radii; d.tiles_touched = fb.g.tiles_touched; d.offsets = fb.g.offsets; d.rows = x.feature_scratch;
        vec = vec && (uintptr_t)x.feature_scratch % 16 == 0;
        if (fv.n == BATCH_VIEWS)
            if (int r = flush()) return named(fn, r);
    }
    return named(fn, flush());
}

size_t tgs_sizeof_view_median(void) { return sizeof(tgs_view_median_t); }

int tgs_median_views(void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views, const tgs_view_median_t* med)
{
    return outputs_views("tgs_median_views", streams, n_streams, P, n_views, views, nullptr, nullptr, med);
}

int tgs_backward_median_views(void* const* streams, int n_streams, int P, int n_views, const tgs_view_t* views, const tgs_view_median_t* med)
{
    static const char* fn = "tgs_backward_median_views";
    int C;
    if (int r = check_views_call(P, n_views, views, nullptr, nullptr, C, med)) return named(fn, r);
    if (int r = check_streams(streams, n_streams, n_views)) return named(fn, r);
    if (P == 0 || !med) return TGS_OK;
    for (int k = 0; k < n_views; k++) {
        tgs_view_median_t m;
        if (int r = read_median(med, k, m)) return named(fn, r);
        const tgs_view_t& w = views[k];
        if (!m.dL_dmedian_depth || w.R == 0) continue;      // (R == 0: no pixel has a median entry; the range pass skips the view as well)
        hipStream_t st = (hipStream_t)streams[k % n_streams];
        const Frame f = frame_facts(P, w.width, w.height, w.R, w.geom_buffer, w.binning_buffer, w.img_buffer);
        if (!f.sizes_ok) return fail(TGS_ERR_INVALID, "%s: view %d: bad sizes", fn, k);
        if (!f.grid_ok) return fail(TGS_ERR_INVALID, "%s: view %d: image too large", fn, k);
        if (!f.buffers_ok) return fail(TGS_ERR_INVALID, "%s: view %d: NULL required pointer", fn, k);
        if (int r = stage(st, TGS_STAGE_RENDER_BWD, "median_bwd", 0, [&] {
                launch_median_bwd(st, f.fb.s, f.fb.b, w.width, w.height, f.v.gx(), (uint32_t)f.v.T(), (size_t)w.R, m.out_pos, m.dL_dmedian_depth, m.dz_scratch); }))
            return named(fn, r);
    }
    return TGS_OK;
}

int tgs_backward_batch_median_range(void* stream, int P, int n_views, const tgs_view_t* views, const tgs_view_median_t* med, float* dL_dmean3D, int first, int count)
{
    static const char* fn = "tgs_backward_batch_median_range";
    int C;
    if (int r = check_views_call(P, n_views, views, nullptr, nullptr, C, med)) return named(fn, r);
    if (!med) return TGS_OK;
    return z_path_range(fn, (hipStream_t)stream, P, n_views, views, dL_dmean3D, first, count, [&](int k, const float*& rows) -> int {
        tgs_view_median_t m;
        if (int r = read_median(med, k, m)) return r;
        rows = m.dL_dmedian_depth ? m.dz_scratch : nullptr;
        return TGS_OK;
    });
}

int tgs_surface_votes(void* stream, int P, int64_t n, const int32_t* index, const uint8_t* mask, int32_t* seen, int32_t* hits)
{
    static const char* fn = "tgs_surface_votes";
    g_err[0] = 0;
    if (P < 0 || n < 0) return fail(TGS_ERR_INVALID, "%s: bad sizes P=%d n=%lld", fn, P, (long long)n);
    if (P == 0 || n == 0) return TGS_OK;
    if (!index || !seen) return fail(TGS_ERR_INVALID, "%s: NULL required pointer (index, seen)", fn);
    if (mask && !hits) return fail(TGS_ERR_INVALID, "%s: a mask without hits", fn);
    if ((n + 255) / 256 > 0x7fffffffll) return fail(TGS_ERR_INVALID, "%s: n=%lld is too large for one call", fn, (long long)n);
    launch_surface_votes((hipStream_t)stream, P, (long long)n, index, mask, seen, hits);
    return hip_status(fn);
}

int tgs_backward_render(void* stream, int P, int64_t R, const float* background, int width, int height, const void* binning_buffer,
                        const void* img_buffer, const float* dL_dpix)
{
    return tgs_backward_render_opt(nullptr, stream, P, R, background, width, height, binning_buffer, img_buffer, dL_dpix);
}

// tgs_backward_render[_alpha]_opt: their arguments as the one view of backward_render_impl
static tgs_view_t render_view(int64_t R, const float* background, int width, int height, const void* binning_buffer, const void* img_buffer, const float* dL_dpix)
{
    tgs_view_t v;
    memset(&v, 0, sizeof(v));
    v.width = width; v.height = height; v.R = R; v.background = background; v.binning_buffer = binning_buffer; v.img_buffer = img_buffer; v.dL_dpix = dL_dpix;
    return v;
}

int tgs_backward_render_opt(const tgs_options_t* o, void* stream, int P, int64_t R, const float* background, int width, int height, const void* binning_buffer,
                            const void* img_buffer, const float* dL_dpix)
{
    return backward_render_impl(resolve_options(o), (hipStream_t)stream, P, render_view(R, background, width, height, binning_buffer, img_buffer, dL_dpix));
}

int tgs_backward_render_alpha_opt(const tgs_options_t* o, void* stream, int P, int64_t R, const float* background, int width, int height,
                                  const void* binning_buffer, const void* img_buffer, const float* dL_dpix, const float* dL_dalpha)
{
    return named("tgs_backward_render_alpha_opt", backward_render_impl(resolve_options(o), (hipStream_t)stream, P,
                                                                       render_view(R, background, width, height, binning_buffer, img_buffer, dL_dpix), dL_dalpha));
}

// tgs_alpha stays apart from open_frame: it reads the image buffer alone, of a frame it knows neither P nor R of (so there is no "nothing
// was blended"), and its launch is linear in the pixels: no tile grid, no grid limit
int tgs_alpha(void* stream, int width, int height, const void* img_buffer, float* out_alpha)
{
    g_err[0] = 0;
    if (width <= 0 || height <= 0) return fail(TGS_ERR_INVALID, "tgs_alpha: bad sizes W=%d H=%d", width, height);
    if (!img_buffer || !out_alpha) return fail(TGS_ERR_INVALID, "tgs_alpha: NULL required pointer");
    const ViewArgs v{nullptr, width, height, nullptr, nullptr, nullptr, 0.f, 0.f};
    ImgState s;
    img_carve(s, (char*)img_buffer, v.N(), v.T());
    launch_alpha((hipStream_t)stream, s, v.N(), out_alpha);
    return hip_status("tgs_alpha");
}

int tgs_depth(void* stream, int P, int width, int height, int64_t R, const void* geom_buffer, const void* binning_buffer, const void* img_buffer, float* out_depth)
{
    Frame f;                                                // nothing blended: the depth is zero (the caller's zeros stand)
    const int go = open_frame(f, "tgs_depth", P, width, height, R, geom_buffer, binning_buffer, img_buffer, out_depth != nullptr);
    if (go <= 0) return go;
    launch_depth_fwd((hipStream_t)stream, f.fb.s, f.fb.b, width, height, f.v.gx(), (uint32_t)f.v.T(), out_depth);
    return hip_status("tgs_depth");
}

int tgs_median(void* stream, int P, int width, int height, int64_t R, const void* geom_buffer, const void* binning_buffer, const void* img_buffer,
               float* out_depth, int32_t* out_index, int32_t* out_pos)
{
    Frame f;                                                // nothing blended: no pixel has a median entry (the caller's 0 / -1 / 0 stand)
    const int go = open_frame(f, "tgs_median", P, width, height, R, geom_buffer, binning_buffer, img_buffer, out_depth && out_index && out_pos);
    if (go <= 0) return go;
    launch_median_fwd((hipStream_t)stream, f.fb.s, f.fb.b, width, height, f.v.gx(), (uint32_t)f.v.T(), out_depth, out_index, out_pos);
    return hip_status("tgs_median");
}

int tgs_backward_median(void* stream, int P, int width, int height, int64_t R, const void* geom_buffer, const void* binning_buffer, const void* img_buffer,
                        const float* viewmatrix, const int* radii, const int32_t* median_pos, const float* dL_dmedian_depth, float* dz_scratch, float* dL_dmean3D)
{
    static const char* fn = "tgs_backward_median";
    hipStream_t st = (hipStream_t)stream;
    Frame f;                                                // nothing blended: no pixel has a median entry, nothing to add
    const int go = open_frame(f, fn, P, width, height, R, geom_buffer, binning_buffer, img_buffer,
                              viewmatrix && radii && median_pos && dL_dmedian_depth && dz_scratch && dL_dmean3D);
    if (go <= 0) return go;
    if (int r = stage(st, TGS_STAGE_RENDER_BWD, "median_bwd", 0, [&] {
            launch_median_bwd(st, f.fb.s, f.fb.b, width, height, f.v.gx(), (uint32_t)f.v.T(), (size_t)R, median_pos, dL_dmedian_depth, dz_scratch); }))
        return named(fn, r);
    // dz . (third row of the view transform), added behind whatever the main backward stored or accumulated on this stream
    return named(fn, stage(st, TGS_STAGE_PREPROCESS_BWD, "median_bwd_gauss", 0, [&] {
        launch_depth_bwd_gauss(st, P, f.fb.s.meta, radii, f.fb.g, viewmatrix, dz_scratch, dL_dmean3D); }));
}

int tgs_features(void* stream, int P, int C, int width, int height, int64_t R, const void* geom_buffer, const void* binning_buffer, const void* img_buffer,
                 const float* features, float* out)
{
    static const char* fn = "tgs_features";
    Frame f;                                                // nothing blended: the map is zero (the caller's zeros stand)
    // (the channel count is looked at behind the sizes and in front of everything else: an empty model with C = 0 is an error)
    const bool bad_C = C < 1 || C > TGS_FEATURE_MAX_CHANNELS;
    const int go = open_frame(f, fn, P, width, height, R, geom_buffer, binning_buffer, img_buffer, features && out);
    if (f.sizes_ok && bad_C) return fail(TGS_ERR_INVALID, "%s: bad channel count C=%d (1 .. %d)", fn, C, TGS_FEATURE_MAX_CHANNELS);
    if (go <= 0) return go;
    launch_feat_fwd((hipStream_t)stream, f.fb.s, f.fb.b, width, height, f.v.gx(), (uint32_t)f.v.T(), P, C, features, out);
    return hip_status(fn);
}

int tgs_backward_batch(void* stream, int P, int D, int M, int n_views, const tgs_view_t* views, const float* means3D, const float* shs,
                       const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp, float* dL_dopacity,
                       float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int accumulate)
{
    return tgs_backward_batch_range(stream, P, D, M, n_views, views, means3D, shs, scales, scale_modifier, rotations, cov3D_precomp, dL_dopacity, dL_dmean3D,
                                    dL_dcov3D, dL_dsh, dL_dscale, dL_drot, accumulate, 0, P);
}

int tgs_backward_batch_range(void* stream, int P, int D, int M, int n_views, const tgs_view_t* views, const float* means3D, const float* shs,
                             const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp, float* dL_dopacity,
                             float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int accumulate, int first, int count)
{
    return tgs_backward_batch_range_planes(stream, P, D, M, n_views, views, means3D, shs, scales, scale_modifier, rotations, cov3D_precomp, dL_dopacity, dL_dmean3D,
                                           dL_dcov3D, dL_dsh, dL_dscale, dL_drot, accumulate, first, count, 0);
}

int tgs_backward_batch_range_planes(void* stream, int P, int D, int M, int n_views, const tgs_view_t* views, const float* means3D, const float* shs,
                                    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp, float* dL_dopacity,
                                    float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int accumulate, int first, int count,
                                    int64_t dsh_plane_stride)
{
    hipStream_t st = (hipStream_t)stream;
    g_err[0] = 0;
    if (P == 0 || n_views == 0 || count == 0) return TGS_OK;
    if (P < 0 || n_views < 0 || !views) return fail(TGS_ERR_INVALID, "bad sizes");
    if (int r = check_gaussian_range(P, first, count)) return r;
    const Model m{P, D, M, means3D, shs, nullptr, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
    const bool has_sh = m.has_sh(), has_sr = m.has_sr();
    if (int r = check_model(m, MODEL_BATCH_BACKWARD)) return r;
    if (!dL_dopacity || !dL_dmean3D || (has_sh && !dL_dsh) || (has_sr && (!dL_dscale || !dL_drot)) || (!has_sr && !dL_dcov3D))
        return fail(TGS_ERR_INVALID, "NULL required pointer");
    if (dsh_plane_stride != 0 && (!has_sh || M != 16 || dsh_plane_stride < 3 * (int64_t)P || dsh_plane_stride % 4 != 0 || ((uintptr_t)dL_dsh & 15u) != 0))
        return fail(TGS_ERR_INVALID, "level-major dL_dsh needs SH colours with M = 16, a plane stride >= 3 P that is a multiple of 4 floats, and a 16-byte aligned dL_dsh");
    BwdIn in = bwd_in(m);
    in.dL_dopacity = dL_dopacity; in.dL_dmean3D = dL_dmean3D; in.dL_dcov3D = has_sr ? nullptr : dL_dcov3D; in.dL_dsh = dL_dsh;
    in.dL_dscale = has_sr ? dL_dscale : nullptr; in.dL_drot = has_sr ? dL_drot : nullptr;
    in.block0 = first / PRE_BLOCK; in.nblocks = (int)n_blocks((size_t)count);
    in.dsh_plane = (long long)dsh_plane_stride;
    for (int v0 = 0; v0 < n_views; v0 += BATCH_VIEWS) {
        BatchViews bv;
        memset(&bv, 0, sizeof(bv));
        bv.n = n_views - v0 < BATCH_VIEWS ? n_views - v0 : BATCH_VIEWS;
        for (int k = 0; k < bv.n; k++) {
            const tgs_view_t& w = views[v0 + k];
            if (int r = check_view(w, v0 + k, VIEW_BATCH_BWD, has_sh)) return r;
            const ViewArgs v = view_args(w);
            const FrameBuffers fb = carve_frame(m.shape(), v, w.R, w.geom_buffer, w.binning_buffer, w.img_buffer);
            BatchView& o = bv.v[k];
            o.cam = v.cam(scale_modifier); o.g = fb.g; o.b = fb.b;
            o.meta = fb.s.meta; o.radii = w.radii; o.dL_dmean2D = w.dL_dmean2D; o.dL_dcolor = has_sh ? nullptr : w.dL_dcolor;
        }
        in.accumulate = (accumulate || v0 > 0) ? 1 : 0;       // later chunks add to what the first one stored
        if (int r = stage(st, TGS_STAGE_PREPROCESS_BWD, "preprocess_bwd_batch", 0, [&] { launch_preprocess_bwd_batch(st, in, bv); })) return r;
    }
    return TGS_OK;
}

int tgs_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present)
{
    hipStream_t st = (hipStream_t)stream;
    g_err[0] = 0;
    (void)projmatrix;       // the reference's x/y frustum test is commented out (auxiliary.h:154)
    if (P == 0) return TGS_OK;
    if (P < 0 || !means3D || !viewmatrix || !present) return fail(TGS_ERR_INVALID, "bad arguments");
    launch_mark_visible(st, P, means3D, viewmatrix, present);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TGS_ERR_HIP, "mark_visible: %s", hipGetErrorString(e));
    return TGS_OK;
}

int64_t tgs_state_field(void* stream, const char* field, int P, int width, int height, int64_t R, int has_sh, int has_scale_rot,
                        const void* geom_buffer, const void* binning_buffer, const void* img_buffer, void* dst, size_t dst_bytes)
{
    hipStream_t st = (hipStream_t)stream;
    g_err[0] = 0;
    const ViewArgs v{nullptr, width, height, nullptr, nullptr, nullptr, 0.f, 0.f};
    const size_t N = v.N(), T = v.T();
    const FrameBuffers fb = carve_frame(GeomShape{(size_t)P, has_sh != 0, has_scale_rot != 0}, v, R, geom_buffer, binning_buffer, img_buffer);
    const GeomState& g = fb.g; const ImgState& s = fb.s; const BinState& b = fb.b;
    const void* src = nullptr; size_t count = 0, esz = 4, stride = 0, rows = 0;   // stride != 0: `rows` rows of `esz` bytes, `stride` apart
    if (!strcmp(field, "n_contrib")) { src = s.n_contrib; count = N; }
    else if (!strcmp(field, "final_T")) { src = s.final_T; count = N; }
    else if (!strcmp(field, "ranges")) { src = s.ranges; count = 2 * T; }
    else if (!strcmp(field, "means2D")) { src = g.pack; count = 2 * (size_t)P; esz = 8; stride = 64; rows = (size_t)P; }
    else if (!strcmp(field, "depths")) { src = g.depth; count = (size_t)P; }
    else if (!strcmp(field, "conic_opacity")) { src = (const char*)g.pack + 8; count = 4 * (size_t)P; esz = 16; stride = 64; rows = (size_t)P; }
    else if (!strcmp(field, "rgb")) { src = (const char*)g.pack + 24; count = 3 * (size_t)P; esz = 12; stride = 64; rows = (size_t)P; }
    else if (!strcmp(field, "tiles_touched")) { src = g.tiles_touched; count = (size_t)P; }
    else if (!strcmp(field, "tile_order")) { src = s.tile_order; count = T; }
    else if (!strcmp(field, "stamps")) { src = s.stamps; count = 8 * T; esz = 8; }
    else if (!strcmp(field, "block_masks")) { src = (const char*)b.recC + 4; count = (size_t)R; esz = 4; stride = 8; rows = (size_t)R; }   // 16-bit culling mask per sorted instance
    else if (!strcmp(field, "quad_masks")) { src = b.qmask; count = (size_t)R; esz = 8; }                               // 64-bit quadrant mask per sorted instance
    else if (!strcmp(field, "point_list")) { src = b.keys; count = (size_t)R; esz = 4; stride = 8; rows = (size_t)R; }   // low 32 bits of each sorted key
    else return fail(TGS_ERR_INVALID, "unknown field %s", field);
    const size_t total = stride ? rows * esz : count * esz;
    if (dst_bytes < total) return fail(TGS_ERR_INVALID, "dst too small for %s", field);
    if (count == 0) return 0;
    if (stride) HIP_TRY(hipMemcpy2DAsync(dst, esz, src, stride, esz, rows, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemcpyAsync(dst, src, total, hipMemcpyDeviceToDevice, st));
    return (int64_t)count;
}

}  // extern "C"
