// tgs_torch_ext.cpp -- the compiled `_C` extension of the drop-in package: torch::Tensor <-> the C ABI of include/tgs_raster.h.
//
// Counterpart of the reference's pybind module (diff-gaussian-rasterization/ext.cpp:15-19) and its glue
// (rasterize_points.cu:35-217, signatures rasterize_points.h:18-67): the same three exports with the same positional
// arguments and return tuples.  Torch is plumbing only -- tensors for device memory (the three state buffers grow through
// resize_ like rasterize_points.cu:27-33), the current HIP stream of the tensors' device -- and everything that computes
// sits behind the C ABI in libtgs_raster.so, which this module links.  Built by plain g++ against the torch / pybind11
// headers (youreditableavatar_amd/build.py: no CUDAExtension, no hipify); host code only, there is no kernel in this file.
#include <torch/extension.h>
// torch on ROCm names its HIP devices "cuda": the guard / stream types that accept that device type are the *MasqueradingAsCUDA ones
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <cstring>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/tgs_raster.h"

namespace {

// resizeFunctional of rasterize_points.cu:27-33 behind the C ABI's one callback: ctx = the three byte tensors.  A FRESH tensor per
// request, not resize_: when the speculative forward asks for the binning buffer a second time (the guess was too small) resize_ would
// copy the whole old buffer -- hundreds of MB of dead data -- into the new one; dropping the old tensor frees it in stream order.
void* alloc_resize(void* ctx, int which, size_t bytes)
{
    torch::Tensor* bufs = static_cast<torch::Tensor*>(ctx);
    if (which < 0 || which > 2) return nullptr;
    bufs[which] = torch::empty({(long long)bytes}, bufs[which].options());
    return bufs[which].data_ptr();
}

[[noreturn]] void raise_last(long long code)
{
    const char* m = tgs_last_error();
    throw std::runtime_error(std::string(m && m[0] ? m : "tgs_raster error") + " (code " + std::to_string(code) + ")");
}

// contiguous fp32 tensor on `dev`; an empty tensor is the reference's "absent" (nullptr: rasterizer_impl.cu:321,389,411 --
// tested by numel() here, not by the data pointer of an empty tensor)
struct Arg {
    torch::Tensor t;
    const float* p = nullptr;
    Arg(const torch::Tensor& x, const c10::Device& dev, const char* name)
    {
        if (!x.defined() || x.numel() == 0) return;
        if (x.scalar_type() != torch::kFloat32) throw std::runtime_error(std::string("expected scalar type Float but found ") + c10::toString(x.scalar_type()) + " for " + name);
        t = (x.device() == dev ? x : x.to(dev)).contiguous();
        p = t.data_ptr<float>();
    }
};

c10::Device require_gpu(const torch::Tensor& means3D)
{
    if (!means3D.is_cuda()) throw std::runtime_error("diff_gaussian_rasterization (MI355X build) has no CPU path: means3D must be on a HIP device");
    return means3D.device();
}

int sh_coeffs(const torch::Tensor& sh) { return (sh.dim() > 1 && sh.size(0) != 0) ? (int)sh.size(1) : 0; }   // rasterize_points.cu:83-87

// keyword-only extensions -> tgs_options_t (None / 0 = library defaults)
tgs_options_t make_options(int64_t tile_bound, c10::optional<bool> pruning, c10::optional<bool> deterministic, int64_t sort_lds_cap, int64_t mid_bound,
                           c10::optional<bool> light_tiles)
{
    tgs_options_t o;
    memset(&o, 0, sizeof(o));
    o.struct_size = (uint32_t)sizeof(o);
    o.instance_pruning = pruning ? (*pruning ? 1 : 0) : -1;
    o.deterministic = deterministic ? (*deterministic ? 1 : 0) : -1;
    o.sort_lds_cap = sort_lds_cap > 0 ? (uint32_t)sort_lds_cap : 0u;
    o.tile_bound = tile_bound > 0 ? tile_bound : 0;
    o.mid_bound = mid_bound > 0 ? mid_bound : 0;
    o.light_tiles = light_tiles ? (*light_tiles ? 1 : 0) : -1;
    return o;
}

// RasterizeGaussiansCUDA (rasterize_points.cu:35-115).  r_capacity / r_guess: the sync-free / speculative forwards of
// include/tgs_raster.h (extensions; None = the reference's protocol).  With r_guess or info=True the tuple has two more elements: the true
// num_rendered and the pair (tiles with instances, tiles with >= 128 instances) (-1 where the call did not read the frame's Meta).  tile_bound / pruning /
// sort_lds_cap travel as an explicit tgs_options_t: nothing process-wide is touched, so threads with different options do not interfere.
py::tuple rasterize_gaussians(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors, const torch::Tensor& opacity,
                              const torch::Tensor& scales, const torch::Tensor& rotations, float scale_modifier, const torch::Tensor& cov3D_precomp,
                              const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, float tan_fovx, float tan_fovy, int image_height,
                              int image_width, const torch::Tensor& sh, int degree, const torch::Tensor& campos, bool prefiltered, bool debug,
                              c10::optional<int64_t> r_capacity, c10::optional<int64_t> r_guess, int64_t tile_bound, c10::optional<bool> pruning,
                              int64_t sort_lds_cap, bool info, int64_t mid_bound, c10::optional<bool> light_tiles)
{
    if (means3D.dim() != 2 || means3D.size(1) != 3) throw std::runtime_error("means3D must have dimensions (num_points, 3)");   // rasterize_points.cu:57-59
    const c10::Device dev = require_gpu(means3D);
    const int P = (int)means3D.size(0), H = image_height, W = image_width, M = sh_coeffs(sh);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(dev);
    torch::Tensor out_color = torch::empty({3, H, W}, f32);
    torch::Tensor radii = torch::empty({P}, f32.dtype(torch::kInt32));
    torch::Tensor bufs[3];
    for (auto& b : bufs) b = torch::empty({0}, f32.dtype(torch::kByte));
    const Arg bg(background, dev, "background"), means(means3D, dev, "means3D"), col(colors, dev, "colors"), op(opacity, dev, "opacity"),
        sc(scales, dev, "scales"), rot(rotations, dev, "rotations"), cov(cov3D_precomp, dev, "cov3D_precomp"), view(viewmatrix, dev, "viewmatrix"),
        proj(projmatrix, dev, "projmatrix"), shs(sh, dev, "sh"), cam(campos, dev, "campos");
    void* stream = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    const tgs_options_t opt = make_options(tile_bound, pruning, c10::nullopt, sort_lds_cap, mid_bound, light_tiles);
    tgs_frame_info_t fi;
    const int mode = r_guess ? TGS_FWD_SPECULATIVE : (r_capacity ? TGS_FWD_ASYNC : TGS_FWD_SYNC);
    int64_t r;
    {
        py::gil_scoped_release nogil;                       // (the allocation callback uses the C++ tensor API only)
        r = tgs_forward_opt(&opt, mode, r_guess ? *r_guess : (r_capacity ? *r_capacity : 0), &fi, alloc_resize, bufs, stream, P, degree, M, bg.p, W, H, means.p, shs.p,
                            col.p, op.p, sc.p, scale_modifier, rot.p, cov.p, view.p, proj.p, cam.p, tan_fovx, tan_fovy, prefiltered, out_color.data_ptr<float>(),
                            P ? radii.data_ptr<int>() : nullptr, debug);
    }
    if (r < 0) raise_last(r);
    if (r_guess || info) return py::make_tuple(r, out_color, radii, bufs[0], bufs[1], bufs[2], fi.num_rendered, py::make_tuple(fi.nonempty_tiles, (int64_t)fi.mid_tiles));
    return py::make_tuple(r, out_color, radii, bufs[0], bufs[1], bufs[2]);
}

// ---- the one-view backward: ONE implementation (BackwardFrame + Upstream -> backward_call) under two exports, rasterize_gaussians_backward
// (gradients stored into fresh tensors, returned) and rasterize_gaussians_backward_into (gradients added into the caller's tensors) ----
// the frame arguments both exports take (rasterize_points.h:42-64), tensors first
struct BackwardFrame {
    const torch::Tensor &background, &means3D, &radii, &colors, &scales, &rotations, &cov3D_precomp, &viewmatrix, &projmatrix, &dL_dout_color, &sh, &campos, &geomBuffer,
        &binningBuffer, &imageBuffer;
    float scale_modifier, tan_fovx, tan_fovy;
    int degree;
    int64_t R;
    bool debug;
    int P() const { return (int)means3D.size(0); }
    int H() const { return (int)dL_dout_color.size(1); }
    int W() const { return (int)dL_dout_color.size(2); }
};

using OptTensor = c10::optional<torch::Tensor>;       // (None = absent)

// an upstream gradient of `count` elements, or absent (None): one sentence for the one mistake, `what` = how the sentence names the count
Arg upstream_arg(const OptTensor& g, int64_t count, const c10::Device& dev, const char* name, const char* what)
{
    if (g && g->numel() != count) throw std::runtime_error(std::string(name) + " must have " + what);
    return Arg(g ? *g : torch::Tensor(), dev, name);
}

// The upstream gradients of a frame's extra outputs (the extension keywords of both exports), validated once, and the scratch that travels with
// them: dz (R floats) with a depth gradient, R * C floats with a feature gradient; the median's call runs behind the main one on the same
// stream, where the depth's dz is free again, so it takes the same buffer.
struct Upstream {
    int C;                      // channels of the feature gradient (0: none)
    Arg dA, dD, dF, feat, dM;
    torch::Tensor mpos, dz, feat_scratch;
    static int channels(const OptTensor& grad_out_features, const OptTensor& features, int P)
    {
        if (!grad_out_features) return 0;
        if (!features || features->dim() != 2 || features->size(0) != P || features->size(1) < 1 || features->size(1) > TGS_FEATURE_MAX_CHANNELS)
            throw std::runtime_error("grad_out_features needs features of shape [P,C], 1 <= C <= " + std::to_string(TGS_FEATURE_MAX_CHANNELS));
        return (int)features->size(1);
    }
    Upstream(const BackwardFrame& f, const c10::Device& dev, const OptTensor& grad_out_alpha, const OptTensor& grad_out_depth, const OptTensor& grad_out_features,
             const OptTensor& features, const OptTensor& grad_out_median, const OptTensor& median_pos)
        : C(channels(grad_out_features, features, f.P())), dA(upstream_arg(grad_out_alpha, (int64_t)f.H() * f.W(), dev, "grad_out_alpha", "H*W elements ([1,H,W])")),
          dD(upstream_arg(grad_out_depth, (int64_t)f.H() * f.W(), dev, "grad_out_depth", "H*W elements ([1,H,W])")),
          dF(upstream_arg(grad_out_features, (int64_t)C * f.H() * f.W(), dev, "grad_out_features", "C*H*W elements ([C,H,W])")),
          feat(C ? *features : torch::Tensor(), dev, "features"),
          dM(upstream_arg(grad_out_median, (int64_t)f.H() * f.W(), dev, "grad_out_median", "H*W elements ([1,H,W])"))
    {
        const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(dev);
        if (dM.p) {
            if (!median_pos || median_pos->numel() != (int64_t)f.H() * f.W() || median_pos->scalar_type() != torch::kInt32)
                throw std::runtime_error("grad_out_median needs median_pos, the int32 map [1,H,W] of median_from_state");
            mpos = (median_pos->device() == dev ? *median_pos : median_pos->to(dev)).contiguous();
        }
        if (dD.p || dM.p) dz = torch::empty({f.R > 0 ? f.R : 1}, f32);
        if (C) feat_scratch = torch::empty({f.R > 0 ? f.R * C : 1}, f32);
    }
};

// where the gradients go, in the library's order; NULL: not wanted (features, conic, colors, cov3D, sh, scales, rotations may be)
struct Dest { float *features, *means2D, *conic, *opacity, *colors, *means3D, *cov3D, *sh, *scales, *rotations; };

// The call of both exports (P != 0): gradients stored (accumulate = 0) or added (1) at `d`.  One library call whatever upstreams there are: NULL / 0
// where one is absent, and without a feature gradient the library takes this for its depth call (tgs_backward_depth_opt, the name its errors then
// carry), without that for the alpha call's, without that for today's.  The median's share is a call of its own behind it, added into d.means3D.
void backward_call(const BackwardFrame& f, const c10::Device& dev, const Upstream& up, const tgs_options_t& opt, int accumulate, const Dest& d)
{
    const Arg bg(f.background, dev, "background"), means(f.means3D, dev, "means3D"), col(f.colors, dev, "colors"), sc(f.scales, dev, "scales"),
        rot(f.rotations, dev, "rotations"), cov(f.cov3D_precomp, dev, "cov3D_precomp"), view(f.viewmatrix, dev, "viewmatrix"), proj(f.projmatrix, dev, "projmatrix"),
        shs(f.sh, dev, "sh"), cam(f.campos, dev, "campos"), dL(f.dL_dout_color, dev, "dL_dout_color");
    const torch::Tensor radii_c = f.radii.contiguous();
    void* stream = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    int r;
    {
        py::gil_scoped_release nogil;
        r = tgs_backward_features_opt(&opt, accumulate, stream, f.P(), f.degree, sh_coeffs(f.sh), f.R, bg.p, f.W(), f.H(), means.p, shs.p, col.p, sc.p, f.scale_modifier, rot.p,
                                      cov.p, view.p, proj.p, cam.p, f.tan_fovx, f.tan_fovy, radii_c.data_ptr<int>(), f.geomBuffer.data_ptr(), f.binningBuffer.data_ptr(),
                                      f.imageBuffer.data_ptr(), dL.p, up.dA.p, up.dD.p, up.dD.p ? up.dz.data_ptr<float>() : nullptr, up.C, up.feat.p, up.dF.p,
                                      up.C ? up.feat_scratch.data_ptr<float>() : nullptr, d.features, d.means2D, d.conic, d.opacity, d.colors, d.means3D, d.cov3D, d.sh,
                                      d.scales, d.rotations, f.debug);
        if (r >= 0 && up.dM.p && f.R > 0)
            r = tgs_backward_median(stream, f.P(), f.W(), f.H(), f.R, f.geomBuffer.data_ptr(), f.binningBuffer.data_ptr(), f.imageBuffer.data_ptr(), view.p,
                                    radii_c.data_ptr<int>(), up.mpos.data_ptr<int>(), up.dM.p, up.dz.data_ptr<float>(), d.means3D);
    }
    if (r < 0) raise_last(r);
}

// RasterizeGaussiansBackwardCUDA (rasterize_points.cu:117-196); return order of :195.  The library writes every element, so the outputs
// are torch::empty (the reference needs nine torch::zeros memsets, :151-159).  with_conic (tests) appends the scratch dL_dconic[P,2,2].
py::tuple rasterize_gaussians_backward(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& colors,
                                       const torch::Tensor& scales, const torch::Tensor& rotations, float scale_modifier, const torch::Tensor& cov3D_precomp,
                                       const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, float tan_fovx, float tan_fovy,
                                       const torch::Tensor& dL_dout_color, const torch::Tensor& sh, int degree, const torch::Tensor& campos,
                                       const torch::Tensor& geomBuffer, int64_t R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, bool debug,
                                       bool with_conic, int64_t tile_bound, c10::optional<bool> deterministic, int64_t mid_bound, c10::optional<bool> light_tiles,
                                       bool need_colors, bool need_cov3D, const OptTensor& grad_out_alpha, const OptTensor& grad_out_depth,
                                       const OptTensor& grad_out_features, const OptTensor& features, const OptTensor& grad_out_median, const OptTensor& median_pos)
{
    // grad_out_median (extension keyword): upstream gradient of the median depth (median_from_state), [1,H,W] or [H,W], with median_pos, the int32 map
    // [1,H,W] that median_from_state returned for this frame; None launches no median kernel, a tensor runs tgs_backward_median behind the main call
    // and adds its share into the returned dL_dmeans3D.  No other gradient gets anything from it.
    // grad_out_features (extension keyword): upstream gradient of the feature map (features_from_state), [C,H,W], with features [P,C]; None launches no
    // feature kernel and returns today's tuple, a tensor travels with a scratch of R * C floats (Upstream), and dL_dfeatures[P,C] is appended to
    // the tuple.
    // grad_out_depth (extension keyword): upstream gradient of the expected depth (depth_from_state), [1,H,W] or [H,W]; None launches no depth kernel,
    // a tensor travels with a scratch of R floats (Upstream).
    // grad_out_alpha (extension keyword): upstream gradient of the accumulated alpha (alpha_from_state), [1,H,W] or [H,W]; None: the colour's alone.
    // need_colors / need_cov3D = false (extension keywords; the reference's signature has neither): the caller will discard dL_dcolors / dL_dcov3D --
    // GaussianRasterizer's backward does when the forward was given shs / scales + rotations (__init__.py:137-152 hands them to inputs that are None) --
    // so they are neither allocated nor written (empty tensors come back); dL_dconic, an intermediate of the reference's two kernels, only on request.
    const c10::Device dev = require_gpu(means3D);
    const int P = (int)means3D.size(0), M = sh_coeffs(sh);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(dev);
    const bool has_sr = scales.numel() != 0;
    const bool want_col = need_colors || M == 0, want_cov = need_cov3D || !has_sr;      // (required outputs on the colors_precomp / cov3D_precomp paths)
    torch::Tensor dL_dmeans3D = torch::empty({P, 3}, f32), dL_dmeans2D = torch::empty({P, 3}, f32), dL_dcolors = torch::empty({want_col ? P : 0, 3}, f32),
                  dL_dconic = torch::empty({with_conic ? P : 0, 2, 2}, f32), dL_dopacity = torch::empty({P, 1}, f32), dL_dcov3D = torch::empty({want_cov ? P : 0, 6}, f32),
                  dL_dsh = torch::empty({P, M, 3}, f32);
    // the reference leaves these at zero on the cov3D_precomp path
    torch::Tensor dL_dscales = has_sr ? torch::empty({P, 3}, f32) : torch::zeros({P, 3}, f32), dL_drotations = has_sr ? torch::empty({P, 4}, f32) : torch::zeros({P, 4}, f32);
    const BackwardFrame f{background, means3D, radii, colors, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, dL_dout_color, sh, campos, geomBuffer,
                          binningBuffer, imageBuffer, scale_modifier, tan_fovx, tan_fovy, degree, R, debug};
    const Upstream up(f, dev, grad_out_alpha, grad_out_depth, grad_out_features, features, grad_out_median, median_pos);
    torch::Tensor dL_dfeatures = up.C ? torch::empty({P, up.C}, f32) : torch::Tensor();
    const auto ptr = [](bool wanted, const torch::Tensor& t) { return wanted ? t.data_ptr<float>() : nullptr; };
    if (P != 0)
        backward_call(f, dev, up, make_options(tile_bound, c10::nullopt, deterministic, 0, mid_bound, light_tiles), 0,
                      {ptr(up.C != 0, dL_dfeatures), ptr(true, dL_dmeans2D), ptr(with_conic, dL_dconic), ptr(true, dL_dopacity), ptr(want_col, dL_dcolors),
                       ptr(true, dL_dmeans3D), ptr(want_cov, dL_dcov3D), ptr(M != 0, dL_dsh), ptr(has_sr, dL_dscales), ptr(has_sr, dL_drotations)});
    py::list out;
    for (const torch::Tensor& g : {dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations}) out.append(g);
    if (with_conic) out.append(dL_dconic);
    if (up.C) out.append(dL_dfeatures);
    return py::tuple(out);
}

// The accumulating export (multi-view extension; _C.rasterize_gaussians_backward_accumulate forwards to it): the same call with accumulate = 1,
// the parameter gradients ADDED into the tensors of `into` -- keys means3D, opacities, sh | colors_precomp, scales + rotations | cov3D_precomp,
// features; a missing key or None is a NULL destination, colors_precomp is not looked at on the SH path nor cov3D_precomp on the scales +
// rotations path -- and dL_dmeans2D[P,3], the only per-view gradient, returned.  The upstream keywords are rasterize_gaussians_backward's; with
// grad_out_features, into["features"] ([P,C]) is required.  An empty model returns the empty [0,3] tensor and looks at nothing else.
torch::Tensor rasterize_gaussians_backward_into(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& colors,
                                                const torch::Tensor& scales, const torch::Tensor& rotations, float scale_modifier, const torch::Tensor& cov3D_precomp,
                                                const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, float tan_fovx, float tan_fovy,
                                                const torch::Tensor& dL_dout_color, const torch::Tensor& sh, int degree, const torch::Tensor& campos,
                                                const torch::Tensor& geomBuffer, int64_t R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, bool debug,
                                                const py::dict& into, int64_t tile_bound, c10::optional<bool> deterministic, int64_t mid_bound,
                                                const OptTensor& grad_out_alpha, const OptTensor& grad_out_depth, const OptTensor& grad_out_features, const OptTensor& features,
                                                const OptTensor& grad_out_median, const OptTensor& median_pos)
{
    const c10::Device dev = require_gpu(means3D);
    const int P = (int)means3D.size(0), M = sh_coeffs(sh);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(dev);
    torch::Tensor dL_dmeans2D = torch::empty({P, 3}, f32);
    if (P == 0) return dL_dmeans2D;
    const BackwardFrame f{background, means3D, radii, colors, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, dL_dout_color, sh, campos, geomBuffer,
                          binningBuffer, imageBuffer, scale_modifier, tan_fovx, tan_fovy, degree, R, debug};
    const Upstream up(f, dev, grad_out_alpha, grad_out_depth, grad_out_features, features, grad_out_median, median_pos);
    std::vector<torch::Tensor> held;                        // (the destinations stay alive while the GIL is released)
    const auto dst = [&](const char* name, std::initializer_list<int64_t> shape) -> float* {
        const py::object g = into.attr("get")(name);
        if (g.is_none()) return nullptr;
        const torch::Tensor t = g.cast<torch::Tensor>();
        if (t.scalar_type() != torch::kFloat32 || t.device() != dev || !t.is_contiguous() || t.sizes() != c10::IntArrayRef(shape))
            throw std::runtime_error(c10::str("accumulation buffer for ", name, " must be a contiguous fp32 tensor of shape ", c10::IntArrayRef(shape), " on ", dev));
        held.push_back(t);
        return t.data_ptr<float>();
    };
    if (up.C && into.attr("get")("features").is_none()) throw std::runtime_error("grad_out_features: into[\"features\"] ([P,C]) is required");
    const bool has_sh = M != 0, has_sr = scales.numel() != 0;
    torch::Tensor dL_dconic = torch::empty({P, 4}, f32);      // (the scratch this call has always handed the library; whether it can go is a measurement of its own)
    backward_call(f, dev, up, make_options(tile_bound, c10::nullopt, deterministic, 0, mid_bound, c10::nullopt), 1,
                  {up.C ? dst("features", {P, up.C}) : nullptr, dL_dmeans2D.data_ptr<float>(), dL_dconic.data_ptr<float>(), dst("opacities", {P, 1}),
                   has_sh ? nullptr : dst("colors_precomp", {P, 3}), dst("means3D", {P, 3}), has_sr ? nullptr : dst("cov3D_precomp", {P, 6}),
                   has_sh ? dst("sh", {P, M, 3}) : nullptr, has_sr ? dst("scales", {P, 3}) : nullptr, has_sr ? dst("rotations", {P, 4}) : nullptr});
    return dL_dmeans2D;
}

// What depth_from_state, median_from_state and features_from_state share: the frame of a finished forward on `dev`, its sizes checked, the
// device made current for the caller's lifetime of this object, and -- unless nothing was blended (P == 0 / R == 0: the caller returns its fill
// and nothing is launched) -- the three state buffers checked against the sizes of such a frame.
struct StateFrame {
    c10::hip::HIPGuardMasqueradingAsCUDA guard;
    torch::TensorOptions f32;
    bool blended;
    void* stream;
    StateFrame(const char* fn, const c10::Device& dev, const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, int P, int H,
               int W, int64_t R)
        : guard(dev), f32(torch::TensorOptions().dtype(torch::kFloat32).device(dev)), blended(P != 0 && R != 0),
          stream((void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream())
    {
        if (!blended) return;
        size_t sizes[3];
        tgs_state_sizes(P, W, H, 0, 0, R, sizes);
        const auto bytes = [](const torch::Tensor& t) { return (size_t)t.numel() * t.element_size(); };
        if (!geomBuffer.is_cuda() || !binningBuffer.is_cuda() || !imageBuffer.is_cuda() || bytes(geomBuffer) < sizes[TGS_BUF_GEOM] ||
            bytes(binningBuffer) < sizes[TGS_BUF_BINNING] || bytes(imageBuffer) < sizes[TGS_BUF_IMAGE])
            throw std::runtime_error(std::string(fn) + ": state buffers smaller than a frame of these sizes");
    }
};

// The accumulated alpha of a finished forward (tgs_alpha): [1,H,W] = 1 - final_T.  The forward of an empty model (P == 0) carves no image
// state -- its buffer is smaller than a frame's -- and has alpha 0 everywhere.  (Apart from StateFrame: it has the image buffer alone and
// neither P nor R, and a buffer that is too small is its empty frame, not an error.)
torch::Tensor alpha_from_state(const torch::Tensor& imageBuffer, int H, int W)
{
    if (!imageBuffer.is_cuda()) throw std::runtime_error("alpha_from_state: imageBuffer must be the image state buffer of a forward, on a HIP device");
    if (H <= 0 || W <= 0) throw std::runtime_error("alpha_from_state: bad sizes");
    const c10::Device dev = imageBuffer.device();
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(dev);
    size_t sizes[3];
    tgs_state_sizes(0, W, H, 0, 0, 0, sizes);
    if ((size_t)imageBuffer.numel() * imageBuffer.element_size() < sizes[TGS_BUF_IMAGE]) return torch::zeros({1, H, W}, f32);
    torch::Tensor alpha = torch::empty({1, H, W}, f32);
    void* stream = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    const int r = tgs_alpha(stream, W, H, imageBuffer.data_ptr(), alpha.data_ptr<float>());
    if (r < 0) raise_last(r);
    return alpha;
}

// The expected depth of a finished forward (tgs_depth): [1,H,W] = sum_i T_i alpha_i z_i over the pairs the colour frame blended.  An empty
// model or a frame without instances (P == 0 / R == 0) has depth 0 everywhere and launches nothing.
torch::Tensor depth_from_state(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, int P, int H, int W, int64_t R)
{
    if (!imageBuffer.is_cuda()) throw std::runtime_error("depth_from_state: the state buffers must be those of a forward, on a HIP device");
    if (P < 0 || H <= 0 || W <= 0 || R < 0) throw std::runtime_error("depth_from_state: bad sizes");
    const StateFrame s("depth_from_state", imageBuffer.device(), geomBuffer, binningBuffer, imageBuffer, P, H, W, R);
    if (!s.blended) return torch::zeros({1, H, W}, s.f32);
    torch::Tensor depth = torch::empty({1, H, W}, s.f32);
    const int r = tgs_depth(s.stream, P, W, H, R, geomBuffer.data_ptr(), binningBuffer.data_ptr(), imageBuffer.data_ptr(), depth.data_ptr<float>());
    if (r < 0) raise_last(r);
    return depth;
}

// The median depth of a finished forward (tgs_median): (median_depth[1,H,W] f32, median_index[1,H,W] i32, median_pos[1,H,W] i32) -- z and Gaussian
// index of the first blended pair after which T < 0.5, and its 1-based position in the tile's list (what the backward reads).  Pixels without
// such a pair, an empty model and a frame without instances: 0 / -1 / 0, and for the latter two nothing is launched.
py::tuple median_from_state(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, int P, int H, int W, int64_t R)
{
    if (!imageBuffer.is_cuda()) throw std::runtime_error("median_from_state: the state buffers must be those of a forward, on a HIP device");
    if (P < 0 || H <= 0 || W <= 0 || R < 0) throw std::runtime_error("median_from_state: bad sizes");
    const StateFrame s("median_from_state", imageBuffer.device(), geomBuffer, binningBuffer, imageBuffer, P, H, W, R);
    const auto i32 = s.f32.dtype(torch::kInt32);
    if (!s.blended) return py::make_tuple(torch::zeros({1, H, W}, s.f32), torch::full({1, H, W}, -1, i32), torch::zeros({1, H, W}, i32));
    torch::Tensor depth = torch::empty({1, H, W}, s.f32), index = torch::empty({1, H, W}, i32), pos = torch::empty({1, H, W}, i32);
    const int r = tgs_median(s.stream, P, W, H, R, geomBuffer.data_ptr(), binningBuffer.data_ptr(), imageBuffer.data_ptr(), depth.data_ptr<float>(), index.data_ptr<int>(),
                             pos.data_ptr<int>());
    if (r < 0) raise_last(r);
    return py::make_tuple(depth, index, pos);
}

// The feature map of a finished forward (tgs_features): [C,H,W] = sum_i T_i alpha_i features[i, :] over the pairs the colour frame blended.
// An empty model or a frame without instances (P == 0 / R == 0) has the map 0 everywhere and launches nothing.
torch::Tensor features_from_state(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const torch::Tensor& features,
                                  int P, int H, int W, int64_t R)
{
    if (!features.is_cuda()) throw std::runtime_error("features_from_state: features must be on a HIP device");
    if (P < 0 || H <= 0 || W <= 0 || R < 0) throw std::runtime_error("features_from_state: bad sizes");
    if (features.dim() != 2 || features.size(0) != P) throw std::runtime_error("features_from_state: features must have shape [P,C]");
    const int C = (int)features.size(1);
    if (C < 1 || C > TGS_FEATURE_MAX_CHANNELS) throw std::runtime_error("features_from_state: features must have 1 .. 16 channels");
    const c10::Device dev = features.device();
    const StateFrame s("features_from_state", dev, geomBuffer, binningBuffer, imageBuffer, P, H, W, R);
    if (!s.blended) return torch::zeros({C, H, W}, s.f32);
    const Arg feat(features, dev, "features");
    torch::Tensor out = torch::empty({C, H, W}, s.f32);
    const int r = tgs_features(s.stream, P, C, W, H, R, geomBuffer.data_ptr(), binningBuffer.data_ptr(), imageBuffer.data_ptr(), feat.p, out.data_ptr<float>());
    if (r < 0) raise_last(r);
    return out;
}

// markVisible (rasterize_points.cu:198-217)
torch::Tensor mark_visible(const torch::Tensor& means3D, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix)
{
    const c10::Device dev = require_gpu(means3D);
    const int P = (int)means3D.size(0);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    torch::Tensor present = torch::zeros({P}, torch::TensorOptions().dtype(torch::kBool).device(dev));
    if (P != 0) {
        const Arg m(means3D, dev, "means3D"), v(viewmatrix, dev, "viewmatrix"), pj(projmatrix, dev, "projmatrix");
        void* stream = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
        const int r = tgs_mark_visible(stream, P, m.p, v.p, pj.p, (uint8_t*)present.data_ptr());
        if (r < 0) raise_last(r);
    }
    return present;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "compiled glue of the MI355X-native diff_gaussian_rasterization: torch::Tensor <-> C ABI (include/tgs_raster.h)";
    m.def("rasterize_gaussians", &rasterize_gaussians, py::arg("background"), py::arg("means3D"), py::arg("colors"), py::arg("opacity"), py::arg("scales"),
          py::arg("rotations"), py::arg("scale_modifier"), py::arg("cov3D_precomp"), py::arg("viewmatrix"), py::arg("projmatrix"), py::arg("tan_fovx"),
          py::arg("tan_fovy"), py::arg("image_height"), py::arg("image_width"), py::arg("sh"), py::arg("degree"), py::arg("campos"), py::arg("prefiltered"),
          py::arg("debug"), py::arg("r_capacity") = py::none(), py::arg("r_guess") = py::none(), py::arg("tile_bound") = 0, py::arg("pruning") = py::none(),
          py::arg("sort_lds_cap") = 0, py::arg("info") = false, py::arg("mid_bound") = 0, py::arg("light_tiles") = py::none());
    // both exports of the one-view backward: the frame arguments, what the export adds (`own`), the upstream keywords
    const auto def_backward = [&m](const char* name, auto fn, auto... own) {
        m.def(name, fn, py::arg("background"), py::arg("means3D"), py::arg("radii"), py::arg("colors"), py::arg("scales"), py::arg("rotations"), py::arg("scale_modifier"),
              py::arg("cov3D_precomp"), py::arg("viewmatrix"), py::arg("projmatrix"), py::arg("tan_fovx"), py::arg("tan_fovy"), py::arg("dL_dout_color"), py::arg("sh"),
              py::arg("degree"), py::arg("campos"), py::arg("geomBuffer"), py::arg("R"), py::arg("binningBuffer"), py::arg("imageBuffer"), py::arg("debug"), own...,
              py::arg("grad_out_alpha") = py::none(), py::arg("grad_out_depth") = py::none(), py::arg("grad_out_features") = py::none(), py::arg("features") = py::none(),
              py::arg("grad_out_median") = py::none(), py::arg("median_pos") = py::none());
    };
    def_backward("rasterize_gaussians_backward", &rasterize_gaussians_backward, py::arg("_with_conic") = false, py::arg("tile_bound") = 0, py::arg("deterministic") = py::none(),
                 py::arg("mid_bound") = 0, py::arg("light_tiles") = py::none(), py::arg("need_colors") = true, py::arg("need_cov3D") = true);
    def_backward("rasterize_gaussians_backward_into", &rasterize_gaussians_backward_into, py::arg("into"), py::arg("tile_bound") = 0, py::arg("deterministic") = py::none(),
                 py::arg("mid_bound") = 0);
    m.def("median_from_state", &median_from_state, py::arg("geomBuffer"), py::arg("binningBuffer"), py::arg("imageBuffer"), py::arg("P"), py::arg("H"), py::arg("W"), py::arg("R"));
    m.def("features_from_state", &features_from_state, py::arg("geomBuffer"), py::arg("binningBuffer"), py::arg("imageBuffer"), py::arg("features"), py::arg("P"),
          py::arg("H"), py::arg("W"), py::arg("R"));
    m.def("depth_from_state", &depth_from_state, py::arg("geomBuffer"), py::arg("binningBuffer"), py::arg("imageBuffer"), py::arg("P"), py::arg("H"), py::arg("W"), py::arg("R"));
    m.def("alpha_from_state", &alpha_from_state, py::arg("imageBuffer"), py::arg("H"), py::arg("W"));
    m.def("mark_visible", &mark_visible);
    m.def("abi_version", []() { return tgs_abi_version(); });
    m.def("compiled_abi_version", []() { return TGS_ABI_VERSION; });      // the header THIS module was compiled against
    m.def("sizeof_view", []() { return sizeof(tgs_view_t); });
    m.def("sizeof_view_features", []() { return sizeof(tgs_view_features_t); });      // the third per-view array of the whole-batch path, as THIS module sees it
}
