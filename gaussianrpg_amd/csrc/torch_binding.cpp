// PyTorch-ROCm extension module `_C`: the operator surface the reference's Python wrapper binds
// (submodules/diff-gaussian-rasterization/ext.cpp:15-20), implemented on top of the C ABI in
// include/grpg_rasterizer.h.  Same four functions, same argument order and return tuples as
// rasterize_points.h:18-88 / rasterize_points.cu:35-306:
//   rasterize_gaussians, rasterize_gaussians_backward, mark_visible, rasterize_gaussians_filter.
// This file is plumbing only (tensor allocation, pointer extraction, stream/device selection);
// it contains no rasterizer arithmetic and has no CPU path: CPU means3D -> error.
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/grpg_rasterizer.h"

namespace {

// Optional inputs arrive as EMPTY (usually CPU) tensors, diff_gaussian_rasterization/__init__.py:
// 207-217; the reference turns them into null data pointers.  Everything else must be fp32 on
// the same HIP device as means3D.
const float* fptr(const torch::Tensor& t, const torch::Tensor& like, const char* name,
                  torch::Tensor& keep) {
  if (!t.defined() || t.numel() == 0) return nullptr;
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32");
  TORCH_CHECK(t.device() == like.device(), name, " must be on ", like.device(), " (got ",
              t.device(), ")");
  keep = t.contiguous();
  return keep.data_ptr<float>();
}

char* resize_blob(size_t bytes, void* user) {   // replaces resizeFunctional, rasterize_points.cu:27-33
  auto* t = static_cast<torch::Tensor*>(user);
  // num_rendered changes a little from frame to frame; round the request up to 1/8-octave steps so
  // the caching allocator keeps handing back the same blocks instead of growing its pools
  // (a pool growth is a hipMalloc, i.e. a device-wide sync in the middle of the frame loop)
  if (bytes > (1u << 20)) {
    size_t step = 1;
    while ((step << 4) <= bytes) step <<= 1;   // step = 2^floor(log2(bytes)) / 8
    bytes = (bytes + step - 1) / step * step;
  }
  t->resize_({static_cast<long long>(bytes)});
  return reinterpret_cast<char*>(t->data_ptr());
}

void require_device(const torch::Tensor& means3D) {
  TORCH_CHECK(means3D.is_cuda(),
              "gaussianrpg_amd: means3D must live on a ROCm/HIP device (torch device 'cuda'); "
              "this rasterizer is MI355X-native and has no CPU path");
}

[[noreturn]] void raise_abi_error(const char* what, int rc) {
  throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) +
                           "): " + grpg_last_error());
}

// ---- the pieces every forward binding is made of: entry checks -> pointers -> outputs -> one call -> tuple ----

// entry checks of the flat bindings, in this order: dims, device, dtype
void check_means3D(const torch::Tensor& means3D) {
  if (means3D.ndimension() != 2 || means3D.size(1) != 3) {
    AT_ERROR("means3D must have dimensions (num_points, 3)");   // rasterize_points.cu:58-60
  }
  require_device(means3D);
  TORCH_CHECK(means3D.scalar_type() == torch::kFloat32, "means3D must be float32");
}

// The camera of a frame.  Two steps, because the checks run in the order of the reference's argument list and
// the flat bindings look at the model's tensors between the background colours and the matrices.
enum class LayerBg { kIfLayered, kAlways };
struct CameraPtrs {
  const float *bg = nullptr, *layer_bg = nullptr, *view = nullptr, *proj = nullptr, *pos = nullptr;
  torch::Tensor keep[5];
  CameraPtrs(const torch::Tensor& like, const torch::Tensor& background, const torch::Tensor* layer_background) {
    bg = fptr(background, like, "background", keep[0]);
    if (layer_background) layer_bg = fptr(*layer_background, like, "layer_background", keep[1]);
  }
  void pose(const torch::Tensor& like, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
            const torch::Tensor& campos) {
    view = fptr(viewmatrix, like, "viewmatrix", keep[2]);
    proj = fptr(projmatrix, like, "projmatrix", keep[3]);
    pos = fptr(campos, like, "campos", keep[4]);
  }
  // forward only (the backward takes what its forward took)
  void require(const LayerBg mode, const bool layered) const {
    if (mode == LayerBg::kAlways) {
      TORCH_CHECK(bg && layer_bg && view && proj && pos, "bg/layer_bg/viewmatrix/projmatrix/campos must be non-empty");
    } else {
      TORCH_CHECK(bg && view && proj && pos, "bg/viewmatrix/projmatrix/campos must be non-empty");
      TORCH_CHECK(!layered || layer_bg, "layer_background must be non-empty in a layered frame");
    }
  }
};

// The flat model of rasterize_gaussians (pack_segments below is the composed counterpart).
struct FlatModelPtrs {
  const float *means, *sh, *colors, *semantics = nullptr, *opacity, *scales, *rotations, *cov3D;
  int P, M = 0;
  torch::Tensor keep[8];
};
FlatModelPtrs flat_model_ptrs(const torch::Tensor& means3D, const torch::Tensor& sh, const torch::Tensor& colors,
                              const torch::Tensor* semantics, const torch::Tensor& opacity,
                              const torch::Tensor& scales, const torch::Tensor& rotations,
                              const torch::Tensor& cov3D_precomp) {
  FlatModelPtrs g;
  g.P = means3D.size(0);
  if (sh.size(0) != 0) g.M = sh.size(1);   // rasterize_points.cu:88-92
  g.means = fptr(means3D, means3D, "means3D", g.keep[0]);
  g.sh = fptr(sh, means3D, "sh", g.keep[1]);
  g.colors = fptr(colors, means3D, "colors_precomp", g.keep[2]);
  if (semantics) g.semantics = fptr(*semantics, means3D, "semantics", g.keep[3]);
  g.opacity = fptr(opacity, means3D, "opacities", g.keep[4]);
  g.scales = fptr(scales, means3D, "scales", g.keep[5]);
  g.rotations = fptr(rotations, means3D, "rotations", g.keep[6]);
  g.cov3D = fptr(cov3D_precomp, means3D, "cov3D_precomp", g.keep[7]);
  return g;
}

// layer_class: uint8 / bool [P] on the device, != 0 = object; NULL for an empty model
const unsigned char* layer_class_ptr(const torch::Tensor& layer_class, const torch::Tensor& means3D,
                                     torch::Tensor& keep) {
  const int64_t P = means3D.size(0);
  TORCH_CHECK(layer_class.numel() == P && layer_class.device() == means3D.device() &&
                  (layer_class.scalar_type() == torch::kUInt8 || layer_class.scalar_type() == torch::kBool),
              "layer_class must be a uint8 / bool tensor of P elements on the device of means3D");
  keep = layer_class.contiguous();
  return P > 0 ? (const unsigned char*)keep.data_ptr() : nullptr;
}

// object_model: uint8 / bool [n] on the HOST, != 0 = the model belongs to the object layer; empty (NULL): actors = objects
const unsigned char* object_model_ptr(const torch::Tensor& object_model, const size_t num_models, torch::Tensor& keep) {
  if (object_model.numel() == 0) return nullptr;
  TORCH_CHECK(object_model.numel() == (int64_t)num_models && !object_model.is_cuda() &&
                  (object_model.scalar_type() == torch::kUInt8 || object_model.scalar_type() == torch::kBool),
              "object_model must be a uint8 / bool HOST tensor with one element per model");
  keep = object_model.contiguous();
  return (const unsigned char*)keep.data_ptr();
}

// returns (num_rendered, rgb8, color, depth, alpha, radii, color_bg, alpha_bg, color_obj, alpha_obj); tensors that
// were not asked for are empty
typedef std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                   torch::Tensor, torch::Tensor, torch::Tensor> FrameResult;

// What a forward call writes: the three private blobs (grown through resize_blob), radii and the planes.  A plane
// that was not asked for is an empty [0] tensor and its pointer is NULL; so are the semantic plane's pointer at
// S == 0 and the radii's at P == 0 (the composition refuses empty models: never there).
struct ForwardOutputs {
  torch::Tensor geom, binning, img, radii, color, depth, alpha, semantic, color_bg, alpha_bg, color_obj, alpha_obj;
  float *p_color, *p_depth, *p_alpha, *p_semantic = nullptr, *p_color_bg, *p_alpha_bg, *p_color_obj, *p_alpha_obj;
  int* p_radii;

  ForwardOutputs(const torch::Tensor& like, const int64_t P, const int H, const int W, const c10::optional<int> S,
                 const bool want_planes, const bool layered) {
    const auto fo = like.options().dtype(torch::kFloat32);
    // every element of these planes is written by the library: no zero-fill pass needed
    auto plane = [&](const bool wanted, const int channels, float*& p) {
      torch::Tensor t = wanted ? torch::empty({channels, H, W}, fo) : torch::empty({0}, fo);
      p = wanted ? t.data_ptr<float>() : nullptr;
      return t;
    };
    color = plane(want_planes, GRPG_NUM_CHANNELS, p_color);
    depth = plane(want_planes, 1, p_depth);
    alpha = plane(want_planes, 1, p_alpha);
    if (S.has_value()) {
      semantic = torch::empty({*S, H, W}, fo);
      if (*S > 0) p_semantic = semantic.data_ptr<float>();
    }
    color_bg = plane(layered, GRPG_NUM_CHANNELS, p_color_bg);
    alpha_bg = plane(layered, 1, p_alpha_bg);
    color_obj = plane(layered, GRPG_NUM_CHANNELS, p_color_obj);
    alpha_obj = plane(layered, 1, p_alpha_obj);
    radii = torch::empty({P}, like.options().dtype(torch::kInt32));
    p_radii = P > 0 ? radii.data_ptr<int>() : nullptr;
    const auto byte_opts = like.options().dtype(torch::kByte);
    geom = torch::empty({0}, byte_opts);
    binning = torch::empty({0}, byte_opts);
    img = torch::empty({0}, byte_opts);
  }
  // rasterize_gaussians (rasterize_points.cu:35-124)
  auto flat(const int n) const { return std::make_tuple(n, color, depth, alpha, semantic, radii, geom, binning, img); }
  auto composed(const int n) const { return std::make_tuple(n, color, depth, alpha, radii, geom, binning, img); }
  auto layers(const int n) const {
    return std::make_tuple(n, color, depth, alpha, radii, color_bg, alpha_bg, color_obj, alpha_obj);
  }
  FrameResult frame(const int n, const torch::Tensor& rgb8) const {
    return std::make_tuple(n, rgb8, color, depth, alpha, radii, color_bg, alpha_bg, color_obj, alpha_obj);
  }
};

// What a backward call gets back from its forward -- radii and the three blobs -- and the upstream gradients of
// the planes.
struct SavedState {
  const float *dcolor, *ddepth, *dalpha, *dsemantic = nullptr;
  int* radii;
  char *geom, *binning, *img;
  torch::Tensor keep[8];
  SavedState(const torch::Tensor& like, const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_depth,
             const torch::Tensor& dL_dout_alpha, const torch::Tensor* dL_dout_semantic, const torch::Tensor& radii_in,
             const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer) {
    dcolor = fptr(dL_dout_color, like, "dL_dout_color", keep[0]);
    ddepth = fptr(dL_dout_depth, like, "dL_dout_depth", keep[1]);
    dalpha = fptr(dL_dout_alpha, like, "dL_dout_alpha", keep[2]);
    if (dL_dout_semantic) dsemantic = fptr(*dL_dout_semantic, like, "dL_dout_semantic", keep[3]);
    TORCH_CHECK(radii_in.scalar_type() == torch::kInt32 && radii_in.device() == like.device(),
                "radii must be int32 on the device");
    radii = (keep[4] = radii_in.contiguous()).data_ptr<int>();
    geom = reinterpret_cast<char*>((keep[5] = geomBuffer.contiguous()).data_ptr());
    binning = reinterpret_cast<char*>((keep[6] = binningBuffer.contiguous()).data_ptr());
    img = reinterpret_cast<char*>((keep[7] = imageBuffer.contiguous()).data_ptr());
  }
};

// One forward call of the C ABI on the current stream.  The call blocks once on the stream (num_rendered
// read-back): let other Python threads drive their own streams meanwhile.  The blob callbacks only touch ATen,
// never Python objects.
template <class Call>
int run(const char* what, Call&& call) {
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  int rendered;
  {
    pybind11::gil_scoped_release nogil;
    rendered = call((void*)stream);
  }
  if (rendered < 0) raise_abi_error(what, rendered);
  return rendered;
}

}  // namespace

std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansImpl(const unsigned flags, int* ticket /* non-NULL: deferred frame */,
                   const torch::Tensor& background, const torch::Tensor& means3D,
                   const torch::Tensor& colors, const torch::Tensor& semantics,
                   const torch::Tensor& opacity, const torch::Tensor& scales,
                   const torch::Tensor& rotations, const float scale_modifier,
                   const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                   const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                   const int image_height, const int image_width, const torch::Tensor& sh,
                   const int degree, const torch::Tensor& campos, const bool prefiltered,
                   const bool debug) {
  check_means3D(means3D);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
  const int H = image_height, W = image_width;
  TORCH_CHECK(semantics.dim() == 2, "semantics must be [P,S]");
  const int S = semantics.size(1);
  CameraPtrs cam(means3D, background, nullptr);
  const FlatModelPtrs g = flat_model_ptrs(means3D, sh, colors, &semantics, opacity, scales, rotations, cov3D_precomp);
  cam.pose(means3D, viewmatrix, projmatrix, campos);
  cam.require(LayerBg::kIfLayered, false);
  ForwardOutputs o(means3D, g.P, H, W, S, true, false);
  const int rendered = run("grpg_forward", [&](void* stream) {
    if (ticket)
      return grpg_forward_deferred(
          resize_blob, &o.geom, resize_blob, &o.binning, resize_blob, &o.img, g.P, degree, g.M, S, cam.bg, W, H,
          g.means, g.sh, g.colors, g.semantics, g.opacity, g.scales, scale_modifier, g.rotations, g.cov3D, cam.view,
          cam.proj, cam.pos, tan_fovx, tan_fovy, prefiltered ? 1 : 0, o.p_color, o.p_depth, o.p_alpha, o.p_semantic,
          o.p_radii, debug ? 1 : 0, stream, flags, ticket);
    return grpg_forward_flags(
        resize_blob, &o.geom, resize_blob, &o.binning, resize_blob, &o.img, g.P, degree, g.M, S, cam.bg, W, H,
        g.means, g.sh, g.colors, g.semantics, g.opacity, g.scales, scale_modifier, g.rotations, g.cov3D, cam.view,
        cam.proj, cam.pos, tan_fovx, tan_fovy, prefiltered ? 1 : 0, o.p_color, o.p_depth, o.p_alpha, o.p_semantic,
        o.p_radii, debug ? 1 : 0, stream, flags);
  });
  return o.flat(rendered);
}

#define GRPG_RASTERIZE_ARGS                                                                        \
  const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,      \
      const torch::Tensor &semantics, const torch::Tensor &opacity, const torch::Tensor &scales,   \
      const torch::Tensor &rotations, const float scale_modifier, const torch::Tensor &cov3D_precomp, \
      const torch::Tensor &viewmatrix, const torch::Tensor &projmatrix, const float tan_fovx,      \
      const float tan_fovy, const int image_height, const int image_width, const torch::Tensor &sh, \
      const int degree, const torch::Tensor &campos, const bool prefiltered, const bool debug
#define GRPG_RASTERIZE_PASS                                                                        \
  background, means3D, colors, semantics, opacity, scales, rotations, scale_modifier, cov3D_precomp, \
      viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,   \
      prefiltered, debug

// the reference's entry point (rasterize_points.cu:35-124): blobs valid for the backward
auto RasterizeGaussians(GRPG_RASTERIZE_ARGS) { return RasterizeGaussiansImpl(0u, nullptr, GRPG_RASTERIZE_PASS); }
// same call when no backward can follow (additive): n_contrib is not produced
auto RasterizeGaussiansEval(GRPG_RASTERIZE_ARGS) {
  return RasterizeGaussiansImpl(GRPG_FORWARD_NO_BACKWARD, nullptr, GRPG_RASTERIZE_PASS);
}
// ... and without the per-frame wait for num_rendered (additive; grpg_forward_deferred): returns
// (ticket, color, depth, alpha, semantic, radii); the outputs may be consumed by further work on
// the stream, but are only KNOWN good once frame_status(ticket) says so
auto RasterizeGaussiansEvalDeferred(GRPG_RASTERIZE_ARGS) {
  int ticket = -1;
  auto r = RasterizeGaussiansImpl(GRPG_FORWARD_NO_BACKWARD, &ticket, GRPG_RASTERIZE_PASS);
  return std::make_tuple(ticket, std::get<1>(r), std::get<2>(r), std::get<3>(r), std::get<4>(r),
                         std::get<5>(r));
}
// Layered frame (additive; grpg_forward_layers): the composition + the background-only and objects-only
// planes of StreetGaussianRenderer.render_all from one pass.  layer_class: uint8 / bool [P], != 0 = object.
// returns (num_rendered, color, depth, alpha, radii, color_bg, alpha_bg, color_obj, alpha_obj)
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor>
RasterizeGaussiansLayers(const torch::Tensor& background, const torch::Tensor& layer_background,
                         const torch::Tensor& layer_class, const torch::Tensor& means3D,
                         const torch::Tensor& colors, const torch::Tensor& opacity, const torch::Tensor& scales,
                         const torch::Tensor& rotations, const float scale_modifier,
                         const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                         const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                         const int image_height, const int image_width, const torch::Tensor& sh,
                         const int degree, const torch::Tensor& campos, const bool debug) {
  check_means3D(means3D);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
  const int H = image_height, W = image_width;
  torch::Tensor k_cls;
  const unsigned char* p_cls = layer_class_ptr(layer_class, means3D, k_cls);
  CameraPtrs cam(means3D, background, &layer_background);
  const FlatModelPtrs g = flat_model_ptrs(means3D, sh, colors, nullptr, opacity, scales, rotations, cov3D_precomp);
  cam.pose(means3D, viewmatrix, projmatrix, campos);
  cam.require(LayerBg::kAlways, true);
  ForwardOutputs o(means3D, g.P, H, W, c10::nullopt, true, true);
  const int rendered = run("grpg_forward_layers", [&](void* stream) {
    return grpg_forward_layers(
        resize_blob, &o.geom, resize_blob, &o.binning, resize_blob, &o.img, g.P, degree, g.M, cam.bg, W, H, g.means,
        g.sh, g.colors, g.opacity, g.scales, scale_modifier, g.rotations, g.cov3D, cam.view, cam.proj, cam.pos,
        tan_fovx, tan_fovy, p_cls, cam.layer_bg, o.p_color, o.p_depth, o.p_alpha, o.p_color_bg, o.p_alpha_bg,
        o.p_color_obj, o.p_alpha_obj, o.p_radii, debug ? 1 : 0, stream);
  });
  return o.layers(rendered);
}

// ---- the frame epilogue (grpg_forward_frame / grpg_forward_composed_frame, ABI 6; host destination: ABI 7) ----
// sky_cube: [6,res,res,3] float32 on the device, or an empty tensor (no sky composite); ray_matrix: 9 floats, CPU
// (taken by value) or device (read by the kernel: no host round trip).
struct EpilogueArgs {
  grpg_frame_epilogue e;
  torch::Tensor k_cube, k_rm, rgb8;
  // colour correction inside the epilogue (grpg_bind_frame_correction): 12 floats on the frame's device, or none
  torch::Tensor k_affine;
  const float* affine = nullptr;
  // binds the matrix for the frame call that follows in the same scaffold
  int bind() const { return affine ? grpg_bind_frame_correction(affine) : GRPG_OK; }
};
// affine: float32, 12 elements ([3,4] row-major) on the frame's device; a contiguous view such as affine_trans[id] is
// taken as it is (no copy, no host read), anything else is made contiguous like _C.color_correct's
static void set_frame_affine(EpilogueArgs& a, const torch::Tensor& like, const c10::optional<torch::Tensor>& affine) {
  if (!affine.has_value() || !affine->defined()) return;
  TORCH_CHECK(affine->device() == like.device() && affine->scalar_type() == torch::kFloat32 && affine->numel() == 12,
              "forward_frame: affine must be a float32 tensor [3,4] on the image's device");
  a.k_affine = affine->contiguous();
  a.affine = a.k_affine.data_ptr<float>();
}
static void make_epilogue(EpilogueArgs& a, const torch::Tensor& like, const torch::Tensor& sky_cube,
                          const torch::Tensor& ray_matrix, const float sky_fill, const bool clamp, const bool want_rgb8,
                          const bool truncate, const c10::optional<torch::Tensor>& out_rgb8, const int H, const int W) {
  a.e = grpg_frame_epilogue{nullptr, 0, nullptr, 0, sky_fill, clamp ? 1 : 0, nullptr, truncate ? 1 : 0, 0};
  if (sky_cube.defined() && sky_cube.numel() != 0) {
    TORCH_CHECK(sky_cube.dim() == 4 && sky_cube.size(0) == 6 && sky_cube.size(1) == sky_cube.size(2) &&
                    sky_cube.size(3) == 3 && sky_cube.scalar_type() == torch::kFloat32 && sky_cube.device() == like.device(),
                "sky_cube must be a float32 [6,res,res,3] tensor on the frame's device");
    TORCH_CHECK(ray_matrix.defined() && ray_matrix.numel() == 9 && ray_matrix.scalar_type() == torch::kFloat32,
                "ray_matrix must hold 9 float32 values (row-major R^T K^-1)");
    a.k_cube = sky_cube.contiguous();
    a.k_rm = ray_matrix.contiguous();
    if (a.k_rm.is_cuda()) TORCH_CHECK(a.k_rm.device() == like.device(), "ray_matrix on another device");
    a.e.sky_cube = a.k_cube.data_ptr<float>();
    a.e.sky_res = (int)a.k_cube.size(1);
    a.e.ray_matrix = a.k_rm.data_ptr<float>();
    a.e.ray_matrix_on_device = a.k_rm.is_cuda() ? 1 : 0;
  }
  if (want_rgb8) {
    if (out_rgb8.has_value() && out_rgb8->defined()) {
      // a PINNED host tensor is a destination too (ABI 7: the epilogue stores the bytes through the link while the
      // render runs; the caller synchronises with the stream before reading, as after a non_blocking copy)
      const bool on_host = out_rgb8->is_cpu();
      TORCH_CHECK(out_rgb8->scalar_type() == torch::kByte && out_rgb8->numel() == (int64_t)3 * H * W &&
                      out_rgb8->is_contiguous() &&
                      (on_host ? out_rgb8->is_pinned() : out_rgb8->device() == like.device()),
                  "out must be a contiguous uint8 tensor of H*W*3 elements on the frame's device, or in pinned host "
                  "memory (Tensor.pin_memory())");
      a.rgb8 = *out_rgb8;
      a.e.out_rgb8_on_host = on_host ? 1 : 0;
    } else {
      a.rgb8 = torch::empty({H, W, 3}, like.options().dtype(torch::kByte));
    }
    a.e.out_rgb8 = a.rgb8.data_ptr<unsigned char>();
  } else {
    a.rgb8 = torch::empty({0}, like.options().dtype(torch::kByte));
  }
}
static const char* const kFrameAsksForNothing = "forward_frame: ask for the float planes, the rgb8 frame, or both";

FrameResult RasterizeGaussiansFrame(
    const torch::Tensor& background, const torch::Tensor& layer_background, const torch::Tensor& layer_class,
    const torch::Tensor& means3D, const torch::Tensor& colors, const torch::Tensor& opacity,
    const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier,
    const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
    const float tan_fovx, const float tan_fovy, const int image_height, const int image_width,
    const torch::Tensor& sh, const int degree, const torch::Tensor& campos, const bool debug,
    const torch::Tensor& sky_cube, const torch::Tensor& ray_matrix, const float sky_fill, const bool clamp,
    const bool want_planes, const bool want_rgb8, const bool truncate, const c10::optional<torch::Tensor>& out_rgb8,
    const c10::optional<torch::Tensor>& affine) {
  check_means3D(means3D);
  TORCH_CHECK(want_planes || want_rgb8, kFrameAsksForNothing);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
  const int H = image_height, W = image_width;
  const bool layered = layer_class.defined() && layer_class.numel() != 0;
  torch::Tensor k_cls;
  const unsigned char* p_cls = layered ? layer_class_ptr(layer_class, means3D, k_cls) : nullptr;
  CameraPtrs cam(means3D, background, &layer_background);
  const FlatModelPtrs g = flat_model_ptrs(means3D, sh, colors, nullptr, opacity, scales, rotations, cov3D_precomp);
  cam.pose(means3D, viewmatrix, projmatrix, campos);
  cam.require(LayerBg::kIfLayered, layered);
  EpilogueArgs ea;
  make_epilogue(ea, means3D, sky_cube, ray_matrix, sky_fill, clamp, want_rgb8, truncate, out_rgb8, H, W);
  set_frame_affine(ea, means3D, affine);
  ForwardOutputs o(means3D, g.P, H, W, c10::nullopt, want_planes, layered);
  const int rendered = run("grpg_forward_frame", [&](void* stream) {
    if (int rc = ea.bind()) return rc;
    return grpg_forward_frame(
        resize_blob, &o.geom, resize_blob, &o.binning, resize_blob, &o.img, g.P, degree, g.M, cam.bg, W, H, g.means,
        g.sh, g.colors, g.opacity, g.scales, scale_modifier, g.rotations, g.cov3D, cam.view, cam.proj, cam.pos,
        tan_fovx, tan_fovy, p_cls, cam.layer_bg, o.p_color, o.p_depth, o.p_alpha, o.p_color_bg, o.p_alpha_bg,
        o.p_color_obj, o.p_alpha_obj, o.p_radii, debug ? 1 : 0, stream, &ea.e);
  });
  return o.frame(rendered, ea.rgb8);
}

// (ok, num_rendered): ok = 1 valid, 0 the frame must be rendered again, -1 not ready (wait = false)
std::tuple<int, int> FrameStatus(const int ticket, const bool wait) {
  int R = 0, rc;
  {
    pybind11::gil_scoped_release nogil;
    rc = grpg_frame_status(ticket, wait ? 1 : 0, &R);
  }
  if (rc == GRPG_OK) return std::make_tuple(1, R);
  if (rc == GRPG_ERR_CAPACITY) return std::make_tuple(0, 0);
  if (rc == GRPG_ERR_NOT_READY) return std::make_tuple(-1, 0);
  raise_abi_error("grpg_frame_status", rc);
  return std::make_tuple(0, 0);
}

// full_intermediates: the reference's binding ALWAYS returns dL_dcolors [P,3] and dL_dcov3D [P,6]
// (rasterize_points.cu:166-176,219) -- the per-Gaussian colour gradient and the 3D-covariance
// gradient, real values even when the colours came from SH / the covariance from scale + rotation.
// _C.rasterize_gaussians_backward (the reference's name) does the same.  The autograd Function
// never looks at them unless the corresponding optional input was given, so it calls
// _C.rasterize_gaussians_backward_lean, which does not materialise the unused ones ([0,3] / [0,6]).
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansBackwardImpl(const torch::Tensor& background, const torch::Tensor& means3D,
                           const torch::Tensor& radii, const torch::Tensor& colors,
                           const torch::Tensor& scales, const torch::Tensor& rotations,
                           const float scale_modifier, const torch::Tensor& cov3D_precomp,
                           const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                           const float tan_fovx, const float tan_fovy,
                           const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_depth,
                           const torch::Tensor& dL_dout_alpha,
                           const torch::Tensor& dL_dout_semantic, const torch::Tensor& sh,
                           const int degree, const torch::Tensor& campos,
                           const torch::Tensor& geomBuffer, const int R,
                           const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                           const torch::Tensor& alphas, const torch::Tensor& semantics,
                           const bool debug, const bool full_intermediates) {
  require_device(means3D);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
  const int P = means3D.size(0);
  const int H = dL_dout_color.size(1);   // rasterize_points.cu:156-158
  const int W = dL_dout_color.size(2);
  const int S = dL_dout_semantic.size(0);
  TORCH_CHECK(S <= GRPG_MAX_SEMANTIC_BACKWARD, "rasterize_gaussians_backward supports at most ",
              GRPG_MAX_SEMANTIC_BACKWARD, " semantic channels, got ", S);
  // rasterize_points.cu:159-163 takes M = 0 when sh has no rows; an EMPTY model (P = 0) that still
  // carries shs of shape [0, M, 3] then gets a [0, 0, 3] gradient autograd rejects -- keep M
  int M = 0;
  if (sh.dim() == 3) M = sh.size(1);

  auto o = means3D.options();
  // The reference zero-fills eleven gradient arrays per call (rasterize_points.cu:166-176) because
  // its kernels accumulate into them.  Here the blend backward accumulates into per-Gaussian
  // records inside the geometry blob and the preprocess backward WRITES every element of the
  // non-semantic arrays (zeros for culled Gaussians): they are allocated uninitialised, each as a
  // tensor of its own (autograd's AccumulateGrad can then adopt them as .grad without a copy, which
  // it cannot do with views into a pool -- 92 MB of clones per step at P = 1 M); only dL_dsemantic
  // (float atomics straight into it) is zero-filled.  Gradients of absent optional inputs
  // (colors_precomp, cov3D_precomp) and the two pure intermediates of the reference's binding
  // (dL_dconic, dL_ddepths) are not materialised at all: the library takes NULL for them.
  const bool want_colors = full_intermediates || colors.numel() != 0;
  const bool want_cov = full_intermediates || cov3D_precomp.numel() != 0;
  torch::Tensor dL_dmeans3D = torch::empty({P, 3}, o);
  torch::Tensor dL_dmeans2D = torch::empty({P, 3}, o);
  torch::Tensor dL_dcolors = torch::empty({want_colors ? P : 0, GRPG_NUM_CHANNELS}, o);
  torch::Tensor dL_dopacity = torch::empty({P, 1}, o);
  torch::Tensor dL_dcov3D = torch::empty({want_cov ? P : 0, 6}, o);
  torch::Tensor dL_dsh = torch::empty({P, M, 3}, o);
  torch::Tensor dL_dscales = torch::empty({P, 3}, o);
  torch::Tensor dL_drotations = torch::empty({P, 4}, o);
  torch::Tensor dL_dsemantic = torch::zeros({P, S}, o);

  if (P != 0) {
    CameraPtrs cam(means3D, background, nullptr);
    torch::Tensor k[8];
    const float* p_means = fptr(means3D, means3D, "means3D", k[0]);
    const float* p_sh = fptr(sh, means3D, "sh", k[1]);
    const float* p_col = fptr(colors, means3D, "colors_precomp", k[2]);
    const float* p_sem = fptr(semantics, means3D, "semantics", k[3]);
    const float* p_alpha = fptr(alphas, means3D, "alphas", k[4]);
    const float* p_sc = fptr(scales, means3D, "scales", k[5]);
    const float* p_rot = fptr(rotations, means3D, "rotations", k[6]);
    const float* p_cov = fptr(cov3D_precomp, means3D, "cov3D_precomp", k[7]);
    cam.pose(means3D, viewmatrix, projmatrix, campos);
    const SavedState sv(means3D, dL_dout_color, dL_dout_depth, dL_dout_alpha, &dL_dout_semantic, radii, geomBuffer,
                        binningBuffer, imageBuffer);
    hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
    const int rc = grpg_backward(
        P, degree, M, R, S, cam.bg, W, H, p_means, p_sh, p_col, p_sem, p_alpha, p_sc, scale_modifier,
        p_rot, p_cov, cam.view, cam.proj, cam.pos, tan_fovx, tan_fovy, sv.radii, sv.geom, sv.binning, sv.img,
        sv.dcolor, sv.ddepth, sv.dalpha, sv.dsemantic,
        dL_dmeans2D.data_ptr<float>(), /*dL_dconic=*/nullptr, dL_dopacity.data_ptr<float>(),
        want_colors ? dL_dcolors.data_ptr<float>() : nullptr, /*dL_ddepth=*/nullptr,
        dL_dmeans3D.data_ptr<float>(), want_cov ? dL_dcov3D.data_ptr<float>() : nullptr,
        M > 0 ? dL_dsh.data_ptr<float>() : nullptr,
        dL_dscales.data_ptr<float>(), dL_drotations.data_ptr<float>(),
        S > 0 ? dL_dsemantic.data_ptr<float>() : nullptr, debug ? 1 : 0, (void*)stream);
    if (rc != GRPG_OK) raise_abi_error("grpg_backward", rc);
  }
  return std::make_tuple(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh,
                         dL_dscales, dL_drotations, dL_dsemantic);
}

#define GRPG_BWD_PARAMS                                                                          \
  const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &radii,     \
      const torch::Tensor &colors, const torch::Tensor &scales, const torch::Tensor &rotations,  \
      const float scale_modifier, const torch::Tensor &cov3D_precomp,                            \
      const torch::Tensor &viewmatrix, const torch::Tensor &projmatrix, const float tan_fovx,    \
      const float tan_fovy, const torch::Tensor &dL_dout_color,                                  \
      const torch::Tensor &dL_dout_depth, const torch::Tensor &dL_dout_alpha,                    \
      const torch::Tensor &dL_dout_semantic, const torch::Tensor &sh, const int degree,          \
      const torch::Tensor &campos, const torch::Tensor &geomBuffer, const int R,                 \
      const torch::Tensor &binningBuffer, const torch::Tensor &imageBuffer,                      \
      const torch::Tensor &alphas, const torch::Tensor &semantics, const bool debug
#define GRPG_BWD_ARGS                                                                            \
  background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,           \
      viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_depth, dL_dout_alpha,    \
      dL_dout_semantic, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, alphas,    \
      semantics, debug
// the reference's entry point: shapes exactly as rasterize_points.cu:166-176,219
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansBackward(GRPG_BWD_PARAMS) { return RasterizeGaussiansBackwardImpl(GRPG_BWD_ARGS, true); }
// additive: what the autograd Function calls
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansBackwardLean(GRPG_BWD_PARAMS) { return RasterizeGaussiansBackwardImpl(GRPG_BWD_ARGS, false); }

// The `poses` argument of the composed family: the host table [n,8] alone (every call from before the device poses),
// or the tuple (host table, pose_rot [R,4], pose_trans [R,3], pose_row [n]) -- the last three optional in that sense:
// float32 contiguous tensors on the models' device and a host int32 tensor, -1 = the host table's row holds the pose
// (grpg_bind_device_poses).  One argument, so all ten functions take it wherever they took the table.
struct PoseArg {
  torch::Tensor host, rot, trans, row;   // rot / trans / row undefined: no device poses
};
namespace pybind11 {
namespace detail {
template <>
struct type_caster<PoseArg> {
  PYBIND11_TYPE_CASTER(PoseArg, const_name("Union[Tensor, Tuple[Tensor, Tensor, Tensor, Tensor]]"));
  bool load(handle src, bool) {
    if (THPVariable_Check(src.ptr())) {
      value.host = THPVariable_Unpack(src.ptr());
      return true;
    }
    if (!isinstance<tuple>(src)) return false;
    const tuple t = reinterpret_borrow<tuple>(src);
    if (t.size() != 4) return false;
    torch::Tensor* const dst[4] = {&value.host, &value.rot, &value.trans, &value.row};
    for (size_t i = 0; i < 4; i++) {
      const handle h = t[i];
      if (!THPVariable_Check(h.ptr())) return false;
      *dst[i] = THPVariable_Unpack(h.ptr());
    }
    return true;
  }
  static handle cast(const PoseArg& p, return_value_policy, handle) {   // (never returned; the macro wants one)
    return handle(THPVariable_Wrap(p.host));
  }
};
}  // namespace detail
}  // namespace pybind11

// the model bundle of the composed family (below): per model one tensor of each raw parameter, the flip masks, and
// the two host tables (the first optionally with the device poses, PoseArg)
#define GRPG_MODEL_PARAMS                                                                                 \
  const std::vector<torch::Tensor> &xyz, const std::vector<torch::Tensor> &scaling,                         \
      const std::vector<torch::Tensor> &rotation, const std::vector<torch::Tensor> &opacity,                \
      const std::vector<torch::Tensor> &features_dc, const std::vector<torch::Tensor> &features_rest,       \
      const std::vector<torch::Tensor> &flip, const PoseArg &poses_arg, const torch::Tensor &idft
#define GRPG_MODEL_ARGS xyz, scaling, rotation, opacity, features_dc, features_rest, flip, poses_arg, idft

torch::Tensor markVisible(torch::Tensor& means3D, torch::Tensor& viewmatrix,
                          torch::Tensor& projmatrix) {
  require_device(means3D);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
  const int P = means3D.size(0);
  torch::Tensor present = torch::full({P}, false, means3D.options().dtype(at::kBool));
  if (P != 0) {
    torch::Tensor k[3];
    const float* p_means = fptr(means3D, means3D, "means3D", k[0]);
    const float* p_view = fptr(viewmatrix, means3D, "viewmatrix", k[1]);
    const float* p_proj = fptr(projmatrix, means3D, "projmatrix", k[2]);
    hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
    const int rc = grpg_mark_visible(P, p_means, p_view, p_proj,
                                     reinterpret_cast<unsigned char*>(present.data_ptr<bool>()),
                                     (void*)stream);
    if (rc != GRPG_OK) raise_abi_error("grpg_mark_visible", rc);
  }
  return present;
}

std::tuple<torch::Tensor, torch::Tensor> RasterizeGaussiansFilter(
    const torch::Tensor& means3D, const torch::Tensor& scales, const torch::Tensor& rotations,
    const float scale_modifier, const torch::Tensor& cov3D_precomp,
    const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, const float tan_fovx,
    const float tan_fovy, const int image_height, const int image_width, const bool prefiltered,
    const bool debug) {
  if (means3D.ndimension() != 2 || means3D.size(1) != 3) {
    AT_ERROR("means3D must have dimensions (num_points, 3)");
  }
  require_device(means3D);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
  const int P = means3D.size(0);
  torch::Tensor radii = torch::full({P}, 0, means3D.options().dtype(torch::kInt32));
  torch::Tensor means2D = torch::full({P, 2}, 0, means3D.options());
  if (P != 0) {
    torch::Tensor k[6];
    const float* p_means = fptr(means3D, means3D, "means3D", k[0]);
    const float* p_sc = fptr(scales, means3D, "scales", k[1]);
    const float* p_rot = fptr(rotations, means3D, "rotations", k[2]);
    const float* p_cov = fptr(cov3D_precomp, means3D, "cov3D_precomp", k[3]);
    const float* p_view = fptr(viewmatrix, means3D, "viewmatrix", k[4]);
    const float* p_proj = fptr(projmatrix, means3D, "projmatrix", k[5]);
    hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
    const int rc = grpg_visible_filter(P, 0, image_width, image_height, p_means, p_sc,
                                       scale_modifier, p_rot, p_cov, p_view, p_proj, tan_fovx,
                                       tan_fovy, prefiltered ? 1 : 0, radii.data_ptr<int>(),
                                       means2D.data_ptr<float>(), debug ? 1 : 0, (void*)stream);
    if (rc != GRPG_OK) raise_abi_error("grpg_visible_filter", rc);
  }
  return std::make_tuple(radii, means2D);
}

// ----------------------------------------------------------------------------------------------
// Fused scene-graph composition (additive; include/grpg_rasterizer.h: grpg_forward_composed).
// Per model one tensor each of the RAW parameters, in the reference's concatenation order
// (background first, then the visible actors); `poses` is a CPU float tensor [nseg, 8] =
// (rigid flag, obj_rot w x y z, obj_trans x y z) -- or that tensor with the device poses behind it (PoseArg) --,
// `idft` a CPU float tensor [nseg, GRPG_MAX_FOURIER].
// ----------------------------------------------------------------------------------------------
namespace {

struct SegmentPack {
  std::vector<grpg_model_segment> segs;
  std::vector<torch::Tensor> keep;
  int64_t P = 0;
  int M = 0;
  // device poses (PoseArg): bound right in front of the C call that consumes them -- nothing that can throw may come
  // between, or the binding would wait for another call
  const float *pose_rot = nullptr, *pose_trans = nullptr;
  const int* pose_row = nullptr;
  int bind() const {
    return pose_row ? grpg_bind_device_poses(pose_rot, pose_trans, pose_row, (int)segs.size()) : GRPG_OK;
  }
};

SegmentPack pack_segments(GRPG_MODEL_PARAMS) {
  const torch::Tensor& poses = poses_arg.host;
  const size_t n = xyz.size();
  TORCH_CHECK(flip.size() == n, "one flip mask (or an empty tensor) per model");
  TORCH_CHECK(n > 0 && n <= GRPG_MAX_SEGMENTS, "need 1..", GRPG_MAX_SEGMENTS, " models");
  TORCH_CHECK(scaling.size() == n && rotation.size() == n && opacity.size() == n &&
                  features_dc.size() == n && features_rest.size() == n,
              "one tensor per model in every parameter list");
  TORCH_CHECK(!poses.is_cuda() && poses.scalar_type() == torch::kFloat32 && poses.dim() == 2 &&
                  poses.size(0) == (int64_t)n && poses.size(1) == 8,
              "poses must be a CPU float tensor [num_models, 8]");
  TORCH_CHECK(!idft.is_cuda() && idft.scalar_type() == torch::kFloat32 && idft.dim() == 2 &&
                  idft.size(0) == (int64_t)n && idft.size(1) == GRPG_MAX_FOURIER,
              "idft must be a CPU float tensor [num_models, ", GRPG_MAX_FOURIER, "]");
  const torch::Tensor pc = poses.contiguous(), ic = idft.contiguous();
  SegmentPack pk;
  pk.segs.resize(n);
  const torch::Tensor& like = xyz[0];
  require_device(like);
  for (size_t i = 0; i < n; i++) {
    grpg_model_segment& g = pk.segs[i];
    const int64_t cnt = xyz[i].size(0);
    TORCH_CHECK(cnt > 0, "model ", i, " is empty: leave it out of the lists");
    TORCH_CHECK(xyz[i].dim() == 2 && xyz[i].size(1) == 3 && scaling[i].numel() == cnt * 3 &&
                    rotation[i].numel() == cnt * 4 && opacity[i].numel() == cnt,
                "model ", i, ": xyz [N,3], scaling [N,3], rotation [N,4], opacity [N,1]");
    TORCH_CHECK(features_dc[i].dim() == 3 && features_dc[i].size(0) == cnt && features_dc[i].size(2) == 3,
                "model ", i, ": features_dc must be [N, fourier_dim, 3]");
    const int F = features_dc[i].size(1);
    const int Mi = 1 + (features_rest[i].numel() > 0 ? (int)features_rest[i].size(1) : 0);
    if (i == 0) pk.M = Mi;
    TORCH_CHECK(Mi == pk.M, "all models must carry the same number of SH coefficients");
    torch::Tensor k[6];
    g.xyz = fptr(xyz[i], like, "xyz", k[0]);
    g.scaling = fptr(scaling[i], like, "scaling", k[1]);
    g.rotation = fptr(rotation[i], like, "rotation", k[2]);
    g.opacity = fptr(opacity[i], like, "opacity", k[3]);
    g.features_dc = fptr(features_dc[i], like, "features_dc", k[4]);
    g.features_rest = fptr(features_rest[i], like, "features_rest", k[5]);
    for (auto& t : k) pk.keep.push_back(t);
    g.flip = nullptr;
    if (flip[i].numel() != 0) {   // training symmetry prior: bool / uint8 [N] on the device
      TORCH_CHECK(flip[i].is_cuda() && flip[i].device() == like.device() && flip[i].numel() == cnt &&
                      (flip[i].scalar_type() == torch::kBool || flip[i].scalar_type() == torch::kUInt8),
                  "model ", i, ": flip must be a bool / uint8 device tensor [N]");
      torch::Tensor fc = flip[i].contiguous();
      pk.keep.push_back(fc);
      g.flip = reinterpret_cast<const unsigned char*>(fc.data_ptr());
    }
    g.count = (int)cnt;
    g.fourier_dim = F;
    const float* pr = pc.data_ptr<float>() + 8 * i;
    g.rigid = pr[0] != 0.0f ? 1 : 0;
    for (int q = 0; q < 4; q++) g.obj_rot[q] = pr[1 + q];
    for (int q = 0; q < 3; q++) g.obj_trans[q] = pr[5 + q];
    for (int q = 0; q < GRPG_MAX_FOURIER; q++) g.idft[q] = ic.data_ptr<float>()[GRPG_MAX_FOURIER * i + q];
    pk.P += cnt;
  }
  if (poses_arg.row.defined()) {
    const torch::Tensor &rot = poses_arg.rot, &trans = poses_arg.trans, &row = poses_arg.row;
    TORCH_CHECK(rot.defined() && trans.defined() && rot.is_cuda() && trans.is_cuda() &&
                    rot.device() == like.device() && trans.device() == like.device() &&
                    rot.scalar_type() == torch::kFloat32 && trans.scalar_type() == torch::kFloat32 &&
                    rot.dim() == 2 && rot.size(1) == 4 && trans.dim() == 2 && trans.size(1) == 3 &&
                    rot.size(0) == trans.size(0) && rot.is_contiguous() && trans.is_contiguous(),
                "device poses: pose_rot [R,4] and pose_trans [R,3] must be contiguous float32 tensors on the models' device");
    TORCH_CHECK(!row.is_cuda() && row.scalar_type() == torch::kInt32 && row.dim() == 1 && row.size(0) == (int64_t)n &&
                    row.is_contiguous(),
                "device poses: pose_row must be a contiguous CPU int32 tensor [num_models]");
    const int* r = row.data_ptr<int>();
    for (size_t i = 0; i < n; i++) {
      TORCH_CHECK(r[i] >= -1 && r[i] < rot.size(0), "device poses: pose_row[", i, "] = ", r[i], " is neither -1 nor a row of pose_rot [",
                  rot.size(0), ",4]");
      TORCH_CHECK(r[i] < 0 || pk.segs[i].rigid, "device poses: model ", i, " has a pose row but no posed flag");
    }
    pk.keep.push_back(rot);
    pk.keep.push_back(trans);
    pk.keep.push_back(row);
    pk.pose_rot = rot.data_ptr<float>();
    pk.pose_trans = trans.data_ptr<float>();
    pk.pose_row = r;
  }
  return pk;
}

}  // namespace

std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor>
RasterizeGaussiansComposed(const torch::Tensor& background, GRPG_MODEL_PARAMS,
                           const float scale_modifier, const torch::Tensor& viewmatrix,
                           const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                           const int image_height, const int image_width, const int degree,
                           const torch::Tensor& campos, const bool debug, const bool for_backward) {
  SegmentPack pk = pack_segments(GRPG_MODEL_ARGS);
  const torch::Tensor& like = xyz[0];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  const int H = image_height, W = image_width;
  CameraPtrs cam(like, background, nullptr);
  cam.pose(like, viewmatrix, projmatrix, campos);
  cam.require(LayerBg::kIfLayered, false);
  ForwardOutputs o(like, pk.P, H, W, c10::nullopt, true, false);
  const int rendered = run("grpg_forward_composed", [&](void* stream) {
    if (int rc = pk.bind()) return rc;
    return grpg_forward_composed_flags(
        resize_blob, &o.geom, resize_blob, &o.binning, resize_blob, &o.img, pk.segs.data(), (int)pk.segs.size(),
        degree, pk.M, cam.bg, W, H, scale_modifier, cam.view, cam.proj, cam.pos, tan_fovx, tan_fovy, o.p_color,
        o.p_depth, o.p_alpha, o.p_radii, debug ? 1 : 0, stream, for_backward ? 0u : GRPG_FORWARD_NO_BACKWARD);
  });
  return o.composed(rendered);
}

// Composition + layered frame (grpg_forward_composed_layers): the reference's whole evaluation render of a frame --
// StreetGaussianModel's getters and StreetGaussianRenderer.render_all -- from the models' raw parameters.
// object_model: uint8 [n] on the host, != 0 = the model belongs to the object layer (empty: actors = objects).
// returns (num_rendered, color, depth, alpha, radii, color_bg, alpha_bg, color_obj, alpha_obj)
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor>
RasterizeGaussiansComposedLayers(const torch::Tensor& background, const torch::Tensor& layer_background,
                                 const torch::Tensor& object_model, GRPG_MODEL_PARAMS, const float scale_modifier,
                                 const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                                 const float tan_fovx, const float tan_fovy, const int image_height,
                                 const int image_width, const int degree, const torch::Tensor& campos,
                                 const bool debug) {
  SegmentPack pk = pack_segments(GRPG_MODEL_ARGS);
  const torch::Tensor& like = xyz[0];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  const int H = image_height, W = image_width;
  torch::Tensor k_cls;
  const unsigned char* p_cls = object_model_ptr(object_model, pk.segs.size(), k_cls);
  CameraPtrs cam(like, background, &layer_background);
  cam.pose(like, viewmatrix, projmatrix, campos);
  cam.require(LayerBg::kAlways, true);
  ForwardOutputs o(like, pk.P, H, W, c10::nullopt, true, true);
  const int rendered = run("grpg_forward_composed_layers", [&](void* stream) {
    if (int rc = pk.bind()) return rc;
    return grpg_forward_composed_layers(
        resize_blob, &o.geom, resize_blob, &o.binning, resize_blob, &o.img, pk.segs.data(), (int)pk.segs.size(),
        p_cls, degree, pk.M, cam.bg, cam.layer_bg, W, H, scale_modifier, cam.view, cam.proj, cam.pos, tan_fovx,
        tan_fovy, o.p_color, o.p_depth, o.p_alpha, o.p_color_bg, o.p_alpha_bg, o.p_color_obj, o.p_alpha_obj,
        o.p_radii, debug ? 1 : 0, stream);
  });
  return o.layers(rendered);
}

// The scene-graph frame as one call (grpg_forward_composed_frame): composition + op (+ layers) + sky + clamp + rgb8.
FrameResult RasterizeGaussiansComposedFrame(
    const torch::Tensor& background, const torch::Tensor& layer_background, const torch::Tensor& object_model,
    const bool layered, GRPG_MODEL_PARAMS,
    const float scale_modifier, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
    const float tan_fovx, const float tan_fovy, const int image_height, const int image_width, const int degree,
    const torch::Tensor& campos, const bool debug, const torch::Tensor& sky_cube, const torch::Tensor& ray_matrix,
    const float sky_fill, const bool clamp, const bool want_planes, const bool want_rgb8, const bool truncate,
    const c10::optional<torch::Tensor>& out_rgb8, const c10::optional<torch::Tensor>& affine) {
  SegmentPack pk = pack_segments(GRPG_MODEL_ARGS);
  const torch::Tensor& like = xyz[0];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  TORCH_CHECK(want_planes || want_rgb8, kFrameAsksForNothing);
  const int H = image_height, W = image_width;
  torch::Tensor k_cls;
  const unsigned char* p_cls = layered ? object_model_ptr(object_model, pk.segs.size(), k_cls) : nullptr;
  CameraPtrs cam(like, background, &layer_background);
  cam.pose(like, viewmatrix, projmatrix, campos);
  cam.require(LayerBg::kIfLayered, layered);
  EpilogueArgs ea;
  make_epilogue(ea, like, sky_cube, ray_matrix, sky_fill, clamp, want_rgb8, truncate, out_rgb8, H, W);
  set_frame_affine(ea, like, affine);
  ForwardOutputs o(like, pk.P, H, W, c10::nullopt, want_planes, layered);
  const int rendered = run("grpg_forward_composed_frame", [&](void* stream) {
    if (int rc = pk.bind()) return rc;
    if (int rc = ea.bind()) return rc;
    return grpg_forward_composed_frame(
        resize_blob, &o.geom, resize_blob, &o.binning, resize_blob, &o.img, pk.segs.data(), (int)pk.segs.size(),
        p_cls, degree, pk.M, cam.bg, cam.layer_bg, W, H, scale_modifier, cam.view, cam.proj, cam.pos, tan_fovx,
        tan_fovy, o.p_color, o.p_depth, o.p_alpha, o.p_color_bg, o.p_alpha_bg, o.p_color_obj, o.p_alpha_obj,
        o.p_radii, debug ? 1 : 0, stream, &ea.e);
  });
  return o.frame(rendered, ea.rgb8);
}

// ---- the baked segment tables of a pose tape (grpg_frame_tables_bake / grpg_bind_frame_table): session.FrameSession ----
// What a bound frame needs per call: the device rows, and per frame the host segments its checks read (pointers,
// counts, Fourier dimensions; the poses in them are not looked at) -- built once, so a frame call packs nothing.
struct FrameTables {
  torch::Tensor rows;                     // uint8 [R * 144] on the device
  std::vector<grpg_model_segment> segs;   // [R] host rows, frame after frame
  std::vector<int> first;                 // [T + 1]
  std::vector<int64_t> P;                 // [T]
  std::vector<torch::Tensor> keep;
  torch::Tensor like;                     // a parameter tensor: the device and options of what a frame allocates
  int M = 0;
  int64_t num_frames() const { return (int64_t)P.size(); }
};

// models: the SCENE's models (GRPG_MODEL_PARAMS; poses [n,8] = posed flag and the pose of a row without a pose row,
// idft ignored); frame_first [T+1], row_model [R], row_pose [R] (row of the flattened pose batch, or -1): host ints;
// row_idft [R, GRPG_MAX_FOURIER] host float32; row_class uint8 [R] on the host or empty; pose_rot [*,4] / pose_trans
// [*,3]: the pose batch on the device.
std::shared_ptr<FrameTables> BakeFrameTables(GRPG_MODEL_PARAMS, const std::vector<int>& frame_first,
                                             const std::vector<int>& row_model, const std::vector<int>& row_pose,
                                             const torch::Tensor& row_idft, const torch::Tensor& row_class,
                                             const torch::Tensor& pose_rot, const torch::Tensor& pose_trans) {
  SegmentPack pk = pack_segments(GRPG_MODEL_ARGS);
  const torch::Tensor& like = xyz[0];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  TORCH_CHECK(frame_first.size() >= 2 && frame_first[0] == 0, "frame_first must be [T+1] host ints starting at 0");
  const int T = (int)frame_first.size() - 1;
  for (int k = 0; k < T; k++)
    TORCH_CHECK(frame_first[k + 1] > frame_first[k] && frame_first[k + 1] - frame_first[k] <= GRPG_MAX_SEGMENTS,
                "frame ", k, " needs 1..", GRPG_MAX_SEGMENTS, " rows");
  const int64_t R = frame_first[T];
  TORCH_CHECK((int64_t)row_model.size() == R && (int64_t)row_pose.size() == R, "one model and one pose row per row");
  TORCH_CHECK(!row_idft.is_cuda() && row_idft.scalar_type() == torch::kFloat32 && row_idft.dim() == 2 &&
                  row_idft.size(0) == R && row_idft.size(1) == GRPG_MAX_FOURIER && row_idft.is_contiguous(),
              "row_idft must be a contiguous CPU float tensor [rows, ", GRPG_MAX_FOURIER, "]");
  const unsigned char* p_cls = nullptr;
  if (row_class.defined() && row_class.numel() != 0) {
    TORCH_CHECK(!row_class.is_cuda() && row_class.scalar_type() == torch::kUInt8 && row_class.numel() == R &&
                    row_class.is_contiguous(),
                "row_class must be a contiguous uint8 HOST tensor with one element per row");
    p_cls = row_class.data_ptr<unsigned char>();
  }
  TORCH_CHECK(pose_rot.is_cuda() && pose_trans.is_cuda() && pose_rot.device() == like.device() &&
                  pose_trans.device() == like.device() && pose_rot.scalar_type() == torch::kFloat32 &&
                  pose_trans.scalar_type() == torch::kFloat32 && pose_rot.dim() == 2 && pose_rot.size(1) == 4 &&
                  pose_trans.dim() == 2 && pose_trans.size(1) == 3 && pose_rot.size(0) == pose_trans.size(0) &&
                  pose_rot.is_contiguous() && pose_trans.is_contiguous(),
              "pose_rot [R,4] and pose_trans [R,3] must be contiguous float32 tensors on the models' device");
  const int64_t num_pose_rows = pose_rot.size(0);
  auto ft = std::make_shared<FrameTables>();
  ft->first = frame_first;
  ft->M = pk.M;
  ft->like = like;
  ft->keep = pk.keep;
  ft->segs.resize((size_t)R);
  const float* idft_p = row_idft.data_ptr<float>();
  for (int k = 0; k < T; k++) {
    int64_t P = 0;
    for (int i = frame_first[k]; i < frame_first[k + 1]; i++) {
      TORCH_CHECK(row_model[i] >= 0 && row_model[i] < (int)pk.segs.size(), "row ", i, " names a model outside the scene");
      TORCH_CHECK(row_pose[i] >= -1 && row_pose[i] < num_pose_rows, "row ", i, ": pose row outside the pose batch");
      grpg_model_segment& g = ft->segs[(size_t)i];
      g = pk.segs[(size_t)row_model[i]];
      for (int q = 0; q < GRPG_MAX_FOURIER; q++) g.idft[q] = idft_p[(size_t)GRPG_MAX_FOURIER * i + q];
      P += g.count;
    }
    ft->P.push_back(P);
  }
  ft->rows = torch::empty({(int64_t)grpg_frame_tables_bytes(R)}, like.options().dtype(torch::kByte));
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  int rc;
  {
    pybind11::gil_scoped_release nogil;
    rc = grpg_frame_tables_bake(ft->rows.data_ptr(), pk.segs.data(), (int)pk.segs.size(), frame_first.data(), T,
                                row_model.data(), row_pose.data(), idft_p, p_cls, pose_rot.data_ptr<float>(),
                                pose_trans.data_ptr<float>(), num_pose_rows, (void*)stream);
  }
  if (rc != GRPG_OK) raise_abi_error("grpg_frame_tables_bake", rc);
  return ft;
}

// Frame k of a baked tape as one call: grpg_bind_frame_table + grpg_forward_composed_frame.  The camera tensors and
// the ray matrix are device tensors (views of the session's rows); nothing is packed, filled or uploaded here.
FrameResult RasterizeGaussiansBoundFrame(
    const std::shared_ptr<FrameTables>& ft, const int64_t k, const torch::Tensor& background,
    const torch::Tensor& layer_background, const bool layered, const float scale_modifier,
    const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
    const int image_height, const int image_width, const int degree, const torch::Tensor& campos, const bool debug,
    const torch::Tensor& sky_cube, const torch::Tensor& ray_matrix, const float sky_fill, const bool clamp,
    const bool want_planes, const bool want_rgb8, const bool truncate, const c10::optional<torch::Tensor>& out_rgb8,
    const c10::optional<torch::Tensor>& affine) {
  TORCH_CHECK(ft != nullptr && k >= 0 && k < ft->num_frames(), "frame ", k, " is not one of the baked frames");
  const torch::Tensor& like = ft->like;
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  TORCH_CHECK(want_planes || want_rgb8, kFrameAsksForNothing);
  const int H = image_height, W = image_width;
  CameraPtrs cam(like, background, &layer_background);
  cam.pose(like, viewmatrix, projmatrix, campos);
  cam.require(LayerBg::kIfLayered, layered);
  EpilogueArgs ea;
  make_epilogue(ea, like, sky_cube, ray_matrix, sky_fill, clamp, want_rgb8, truncate, out_rgb8, H, W);
  set_frame_affine(ea, like, affine);
  const int first = ft->first[(size_t)k], nseg = ft->first[(size_t)k + 1] - first;
  const int64_t P = ft->P[(size_t)k];
  const unsigned char* rows = ft->rows.data_ptr<unsigned char>() + (size_t)first * grpg_frame_tables_bytes(1);
  ForwardOutputs o(like, P, H, W, c10::nullopt, want_planes, layered);
  const int rendered = run("grpg_forward_composed_frame", [&](void* stream) {
    if (int rc = ea.bind()) return rc;
    if (int rc = grpg_bind_frame_table(rows, nseg, (int)P)) return rc;
    return grpg_forward_composed_frame(
        resize_blob, &o.geom, resize_blob, &o.binning, resize_blob, &o.img, ft->segs.data() + first, nseg, nullptr,
        degree, ft->M, cam.bg, cam.layer_bg, W, H, scale_modifier, cam.view, cam.proj, cam.pos, tan_fovx, tan_fovy,
        o.p_color, o.p_depth, o.p_alpha, o.p_color_bg, o.p_alpha_bg, o.p_color_obj, o.p_alpha_obj, o.p_radii,
        debug ? 1 : 0, stream, &ea.e);
  });
  return o.frame(rendered, ea.rgb8);
}

// ---- feature planes of a composed frame (grpg_*_features): F = 3 * normals + S channels, normals first ----
namespace {

// The models' semantic arrays: one [N_i,S] float32 device tensor per model, or an empty one (zeros); S is what the
// non-empty ones agree on.  No semantics at all: an empty list.
struct SemanticPack {
  std::vector<const float*> ptrs;
  std::vector<torch::Tensor> keep;
  int S = 0;
};
SemanticPack pack_semantics(const std::vector<torch::Tensor>& semantics, const std::vector<torch::Tensor>& xyz) {
  SemanticPack sp;
  const size_t n = xyz.size();
  TORCH_CHECK(semantics.empty() || semantics.size() == n, "one semantic tensor (or an empty one) per model");
  sp.ptrs.assign(n, nullptr);
  sp.keep.resize(n);
  bool have = false;
  for (size_t i = 0; i < semantics.size(); i++) {
    const torch::Tensor& t = semantics[i];
    if (t.numel() == 0 && !(t.dim() == 2 && t.size(0) == xyz[i].size(0))) continue;   // "no semantics for this model"
    TORCH_CHECK(t.dim() == 2 && t.size(0) == xyz[i].size(0), "model ", i, ": semantics must be [N,S]");
    TORCH_CHECK(!have || t.size(1) == sp.S, "all models must carry the same number of semantic channels (model ", i,
                " has ", t.size(1), ", an earlier one ", sp.S, ")");
    sp.S = t.size(1);
    have = true;
    sp.ptrs[i] = fptr(t, xyz[0], "semantics", sp.keep[i]);
  }
  return sp;
}

// The semantic gradients a backward writes: [N_i,S] for the models that want one (want_semantic[i] and S > 0), an
// empty tensor and a NULL pointer for the others.  Every element is written by the kernel: no zero-fill.
struct SemanticGrads {
  std::vector<torch::Tensor> grads;
  std::vector<float*> ptrs;
  SemanticGrads(const std::vector<torch::Tensor>& xyz, const int S, const std::vector<bool>& want_semantic,
                const torch::TensorOptions& o)
      : grads(xyz.size(), torch::empty({0}, o)), ptrs(xyz.size(), nullptr) {
    TORCH_CHECK(want_semantic.size() == xyz.size(), "one want_semantic flag per model");
    for (size_t i = 0; i < xyz.size(); i++)
      if (want_semantic[i] && S > 0)
        ptrs[i] = (grads[i] = torch::empty({xyz[i].size(0), (int64_t)S}, o)).data_ptr<float>();
  }
};

// The raw-parameter gradients of a frame backward: per model six tensors shaped like the parameters (xyz, scaling,
// rotation, opacity, features_dc, features_rest) and the table of their pointers the C ABI takes.  Every element is
// written by the kernels: no zero-fill.
struct ModelGrads {
  std::vector<torch::Tensor> g[6];
  std::vector<grpg_model_segment_grad> table;
  ModelGrads(const std::vector<torch::Tensor>* const (&params)[6], const torch::TensorOptions& o)
      : table(params[0]->size()) {
    for (int f = 0; f < 6; f++)
      for (const torch::Tensor& t : *params[f]) g[f].push_back(torch::empty(t.sizes(), o));
    for (size_t i = 0; i < table.size(); i++)
      table[i] = grpg_model_segment_grad{g[0][i].data_ptr<float>(), g[1][i].data_ptr<float>(),
                                         g[2][i].data_ptr<float>(), g[3][i].data_ptr<float>(),
                                         g[4][i].data_ptr<float>(),
                                         g[5][i].numel() ? g[5][i].data_ptr<float>() : nullptr};
  }
};

}  // namespace

// composed.compose_features: [P,F]
torch::Tensor ComposeFeatures(GRPG_MODEL_PARAMS,
                              const std::vector<torch::Tensor>& semantics, const bool normals,
                              const torch::Tensor& campos) {
  SegmentPack pk = pack_segments(GRPG_MODEL_ARGS);
  const torch::Tensor& like = xyz[0];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  const SemanticPack sp = pack_semantics(semantics, xyz);
  torch::Tensor k_pos;
  const float* p_pos = fptr(campos, like, "campos", k_pos);
  TORCH_CHECK(!normals || (p_pos && campos.numel() == 3), "normals need campos (3 floats on the device)");
  torch::Tensor features = torch::empty({pk.P, (int64_t)(3 * (normals ? 1 : 0) + sp.S)}, like.options().dtype(torch::kFloat32));
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (int rc = pk.bind()) raise_abi_error("grpg_bind_device_poses", rc);
  const int rc = grpg_compose_features(pk.segs.data(), (int)pk.segs.size(), sp.ptrs.data(), sp.S, normals ? 1 : 0, p_pos,
                                       features.numel() ? features.data_ptr<float>() : nullptr, (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_compose_features", rc);
  return features;
}

// its backward: (dL/d raw rotation per model, dL/d semantic per model ([N_i,S]; empty where want_semantic[i] is
// false), dL_dposes [n,8] with the product path's share in [:, 0:4])
std::tuple<std::vector<torch::Tensor>, std::vector<torch::Tensor>, torch::Tensor>
ComposeFeaturesBackward(GRPG_MODEL_PARAMS,
                        const int S, const std::vector<bool>& want_semantic, const bool normals,
                        const torch::Tensor& campos, const torch::Tensor& dL_dfeatures) {
  SegmentPack pk = pack_segments(GRPG_MODEL_ARGS);
  const torch::Tensor& like = xyz[0];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  const size_t n = xyz.size();
  const int64_t F = 3 * (normals ? 1 : 0) + S;
  auto o = like.options().dtype(torch::kFloat32);
  SemanticGrads sem(xyz, S, want_semantic, o);
  TORCH_CHECK(dL_dfeatures.dim() == 2 && dL_dfeatures.size(0) == pk.P && dL_dfeatures.size(1) == F,
              "dL_dfeatures must be [P,F]");
  torch::Tensor k_pos, k_g;
  const float* p_pos = fptr(campos, like, "campos", k_pos);
  const float* p_g = fptr(dL_dfeatures, like, "dL_dfeatures", k_g);
  TORCH_CHECK(!normals || (p_pos && campos.numel() == 3), "normals need campos (3 floats on the device)");
  std::vector<torch::Tensor> g_rot(n);
  std::vector<float*> p_rot(n, nullptr);
  for (size_t i = 0; i < n; i++) {
    g_rot[i] = torch::zeros(rotation[i].sizes(), o);   // added to
    if (normals) p_rot[i] = g_rot[i].data_ptr<float>();
  }
  torch::Tensor dL_dposes = torch::zeros({(int64_t)n, 8}, o);
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (int rc = pk.bind()) raise_abi_error("grpg_bind_device_poses", rc);
  const int rc = grpg_compose_features_backward(pk.segs.data(), (int)n, S, normals ? 1 : 0, p_pos, p_g, sem.ptrs.data(),
                                                p_rot.data(), dL_dposes.data_ptr<float>(), (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_compose_features_backward", rc);
  return std::make_tuple(g_rot, sem.grads, dL_dposes);
}

// ComposedRasterizer.forward_features: rasterize_gaussians_composed + the feature planes [F,H,W] and the fourth blob.
// returns (num_rendered, color, depth, alpha, features, radii, geom, binning, img, feature blob)
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansComposedFeatures(const torch::Tensor& background, GRPG_MODEL_PARAMS,
                                   const std::vector<torch::Tensor>& semantics,
                                   const bool normals, const float scale_modifier, const torch::Tensor& viewmatrix,
                                   const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                                   const int image_height, const int image_width, const int degree,
                                   const torch::Tensor& campos, const bool debug, const bool for_backward) {
  SegmentPack pk = pack_segments(GRPG_MODEL_ARGS);
  const torch::Tensor& like = xyz[0];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  const SemanticPack sp = pack_semantics(semantics, xyz);
  const int H = image_height, W = image_width, F = 3 * (normals ? 1 : 0) + sp.S;
  CameraPtrs cam(like, background, nullptr);
  cam.pose(like, viewmatrix, projmatrix, campos);
  cam.require(LayerBg::kIfLayered, false);
  ForwardOutputs o(like, pk.P, H, W, F, true, false);
  torch::Tensor feat_blob = torch::empty({0}, like.options().dtype(torch::kByte));
  const int rendered = run("grpg_forward_composed_features", [&](void* stream) {
    if (int rc = pk.bind()) return rc;
    return grpg_forward_composed_features(
        resize_blob, &o.geom, resize_blob, &o.binning, resize_blob, &o.img, resize_blob, &feat_blob, pk.segs.data(),
        (int)pk.segs.size(), sp.ptrs.data(), sp.S, normals ? 1 : 0, degree, pk.M, cam.bg, W, H, scale_modifier,
        cam.view, cam.proj, cam.pos, tan_fovx, tan_fovy, o.p_color, o.p_depth, o.p_alpha, o.p_semantic, o.p_radii,
        debug ? 1 : 0, stream, for_backward ? 0u : GRPG_FORWARD_NO_BACKWARD);
  });
  return std::make_tuple(rendered, o.color, o.depth, o.alpha, o.semantic, o.radii, o.geom, o.binning, o.img, feat_blob);
}

// The training backward of rasterize_gaussians_composed and _composed_features (grpg_backward_composed at F = 0, where
// the feature blob and dL_dout_features are not looked at; grpg_backward_composed_features otherwise): gradients with
// respect to every model's RAW parameter tensors, the semantic arrays ([N_i,S] per model; empty where
// want_semantic[i] is false), means2D [P,3] (densification statistic) and the poses [n,8].
typedef std::tuple<std::vector<torch::Tensor>, std::vector<torch::Tensor>, std::vector<torch::Tensor>,
                   std::vector<torch::Tensor>, std::vector<torch::Tensor>, std::vector<torch::Tensor>,
                   std::vector<torch::Tensor>, torch::Tensor, torch::Tensor> ComposedGrads;
// objects (rasterize_gaussians_composed_objects_backward; NULL: none): {alpha_object, workspace, dL_dout_alpha_object}
// of ComposedRasterizer.forward_objects -- grpg_backward_composed_objects at any F
static ComposedGrads ComposedBackwardImpl(
    const torch::Tensor& background, GRPG_MODEL_PARAMS, const int S, const std::vector<bool>& want_semantic,
    const bool normals, const float scale_modifier, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
    const float tan_fovx, const float tan_fovy, const int degree, const torch::Tensor& campos,
    const torch::Tensor& radii, const torch::Tensor& alphas, const torch::Tensor& geomBuffer, const int R,
    const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const torch::Tensor& featureBuffer,
    const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_depth, const torch::Tensor& dL_dout_alpha,
    const torch::Tensor& dL_dout_features, const bool debug, const torch::Tensor* const (*objects)[3]) {
  SegmentPack pk = pack_segments(GRPG_MODEL_ARGS);
  const torch::Tensor& like = xyz[0];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  const int H = dL_dout_color.size(1), W = dL_dout_color.size(2);
  const int n = (int)xyz.size();
  const int64_t F = 3 * (normals ? 1 : 0) + S;
  auto o = like.options().dtype(torch::kFloat32);
  SemanticGrads sem(xyz, S, want_semantic, o);
  TORCH_CHECK(dL_dout_features.numel() == F * H * W, "dL_dout_features must be [F,H,W]");
  ModelGrads mg({&xyz, &scaling, &rotation, &opacity, &features_dc, &features_rest}, o);
  torch::Tensor dL_dmeans2D = torch::empty({pk.P, 3}, o);
  torch::Tensor dL_dposes = torch::empty({(int64_t)n, 8}, o);
  CameraPtrs cam(like, background, nullptr);
  cam.pose(like, viewmatrix, projmatrix, campos);
  torch::Tensor k_alpha;
  const float* p_alpha = fptr(alphas, like, "alphas", k_alpha);
  const SavedState sv(like, dL_dout_color, dL_dout_depth, dL_dout_alpha, &dL_dout_features, radii, geomBuffer,
                      binningBuffer, imageBuffer);
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (objects) {
    const torch::Tensor &alpha_object = *(*objects)[0], &workspace = *(*objects)[1], &dL_dobj = *(*objects)[2];
    TORCH_CHECK(alpha_object.numel() == (int64_t)H * W && dL_dobj.numel() == (int64_t)H * W,
                "alpha_object and its gradient must be [1,H,W]");
    TORCH_CHECK(workspace.scalar_type() == torch::kByte && workspace.device() == like.device() &&
                    (size_t)workspace.numel() >= grpg_object_alpha_workspace_bytes(W, H),
                "the object-alpha workspace must be the forward's byte tensor");
    torch::Tensor k_obj, k_dobj, k_blob;
    const float* p_obj = fptr(alpha_object, like, "alpha_object", k_obj);
    const float* p_dobj = fptr(dL_dobj, like, "dL_dout_alpha_object", k_dobj);
    const torch::Tensor k_ws = workspace.contiguous();
    torch::Tensor dL_dfeatures = torch::zeros({F > 0 ? pk.P : 0, F}, o);   // the blend backward accumulates into it
    char* p_blob = nullptr;
    if (F > 0) {
      TORCH_CHECK(featureBuffer.scalar_type() == torch::kByte && featureBuffer.device() == like.device(),
                  "the feature blob must be the forward's byte tensor");
      p_blob = reinterpret_cast<char*>((k_blob = featureBuffer.contiguous()).data_ptr());
    }
    if (int rc = pk.bind()) raise_abi_error("grpg_bind_device_poses", rc);
    const int rc = grpg_backward_composed_objects(
        pk.segs.data(), mg.table.data(), n, sem.ptrs.data(), S, normals ? 1 : 0, degree, pk.M, R, cam.bg, W, H,
        scale_modifier, cam.view, cam.proj, cam.pos, tan_fovx, tan_fovy, sv.radii, p_alpha, sv.geom, sv.binning, sv.img,
        p_blob, sv.dcolor, sv.ddepth, sv.dalpha, sv.dsemantic, F > 0 ? dL_dfeatures.data_ptr<float>() : nullptr,
        dL_dmeans2D.data_ptr<float>(), dL_dposes.data_ptr<float>(), p_obj, reinterpret_cast<char*>(k_ws.data_ptr()),
        p_dobj, debug ? 1 : 0, (void*)stream);
    if (rc != GRPG_OK) raise_abi_error("grpg_backward_composed_objects", rc);
  } else if (F == 0) {
    if (int rc = pk.bind()) raise_abi_error("grpg_bind_device_poses", rc);
    const int rc = grpg_backward_composed(
        pk.segs.data(), mg.table.data(), n, degree, pk.M, R, cam.bg, W, H, scale_modifier, cam.view, cam.proj, cam.pos,
        tan_fovx, tan_fovy, sv.radii, p_alpha, sv.geom, sv.binning, sv.img, sv.dcolor, sv.ddepth, sv.dalpha,
        dL_dmeans2D.data_ptr<float>(), dL_dposes.data_ptr<float>(), debug ? 1 : 0, (void*)stream);
    if (rc != GRPG_OK) raise_abi_error("grpg_backward_composed", rc);
  } else {
    torch::Tensor dL_dfeatures = torch::zeros({pk.P, F}, o);   // the blend backward accumulates into it
    TORCH_CHECK(featureBuffer.scalar_type() == torch::kByte && featureBuffer.device() == like.device(),
                "the feature blob must be the forward's byte tensor");
    const torch::Tensor k_blob = featureBuffer.contiguous();
    if (int rc = pk.bind()) raise_abi_error("grpg_bind_device_poses", rc);
    const int rc = grpg_backward_composed_features(
        pk.segs.data(), mg.table.data(), n, sem.ptrs.data(), S, normals ? 1 : 0, degree, pk.M, R, cam.bg, W, H,
        scale_modifier, cam.view, cam.proj, cam.pos, tan_fovx, tan_fovy, sv.radii, p_alpha, sv.geom, sv.binning, sv.img,
        reinterpret_cast<char*>(k_blob.data_ptr()), sv.dcolor, sv.ddepth, sv.dalpha, sv.dsemantic,
        dL_dfeatures.data_ptr<float>(), dL_dmeans2D.data_ptr<float>(), dL_dposes.data_ptr<float>(), debug ? 1 : 0,
        (void*)stream);
    if (rc != GRPG_OK) raise_abi_error("grpg_backward_composed_features", rc);
  }
  return std::make_tuple(mg.g[0], mg.g[1], mg.g[2], mg.g[3], mg.g[4], mg.g[5], sem.grads, dL_dmeans2D, dL_dposes);
}

#define GRPG_COMPOSED_BACKWARD_PARAMS                                                                                \
  const torch::Tensor &background, GRPG_MODEL_PARAMS, const int S, const std::vector<bool>&want_semantic,            \
      const bool normals, const float scale_modifier, const torch::Tensor &viewmatrix,                               \
      const torch::Tensor &projmatrix, const float tan_fovx, const float tan_fovy, const int degree,                 \
      const torch::Tensor &campos, const torch::Tensor &radii, const torch::Tensor &alphas,                          \
      const torch::Tensor &geomBuffer, const int R, const torch::Tensor &binningBuffer,                              \
      const torch::Tensor &imageBuffer, const torch::Tensor &featureBuffer, const torch::Tensor &dL_dout_color,      \
      const torch::Tensor &dL_dout_depth, const torch::Tensor &dL_dout_alpha, const torch::Tensor &dL_dout_features
#define GRPG_COMPOSED_BACKWARD_ARGS                                                                                  \
  background, GRPG_MODEL_ARGS, S, want_semantic, normals, scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy, \
      degree, campos, radii, alphas, geomBuffer, R, binningBuffer, imageBuffer, featureBuffer, dL_dout_color,        \
      dL_dout_depth, dL_dout_alpha, dL_dout_features

ComposedGrads RasterizeGaussiansComposedBackward(GRPG_COMPOSED_BACKWARD_PARAMS, const bool debug) {
  return ComposedBackwardImpl(GRPG_COMPOSED_BACKWARD_ARGS, debug, nullptr);
}

// ComposedRasterizer.forward_objects' backward: the same call with the object-alpha plane's gradient riding along
ComposedGrads RasterizeGaussiansComposedObjectsBackward(GRPG_COMPOSED_BACKWARD_PARAMS,
                                                        const torch::Tensor& alpha_object,
                                                        const torch::Tensor& workspace,
                                                        const torch::Tensor& dL_dout_alpha_object, const bool debug) {
  const torch::Tensor* const objects[3] = {&alpha_object, &workspace, &dL_dout_alpha_object};
  return ComposedBackwardImpl(GRPG_COMPOSED_BACKWARD_ARGS, debug, &objects);
}

// The object-alpha plane of a TRAINING frame (grpg_object_alpha_forward on the blobs its forward left behind).
// layer_class: uint8 / bool [P] on the device, != 0 = object; empty: a composed frame's segment table decides
// (actors = objects).  returns (alpha_object [1,H,W], workspace)
std::tuple<torch::Tensor, torch::Tensor> ObjectAlphaForward(const torch::Tensor& geomBuffer,
                                                            const torch::Tensor& binningBuffer,
                                                            const torch::Tensor& imageBuffer, const int64_t P,
                                                            const torch::Tensor& layer_class, const int image_height,
                                                            const int image_width) {
  const torch::Tensor& like = geomBuffer;
  require_device(like);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  const int H = image_height, W = image_width;
  TORCH_CHECK(H > 0 && W > 0 && P >= 0, "image size must be positive, P not negative");
  for (const torch::Tensor* t : {&geomBuffer, &binningBuffer, &imageBuffer})
    TORCH_CHECK(t->scalar_type() == torch::kByte && t->device() == like.device() && t->is_contiguous(),
                "the state buffers must be the forward's byte tensors");
  torch::Tensor k_cls;
  const unsigned char* p_cls = nullptr;
  if (layer_class.numel() != 0) {
    TORCH_CHECK(layer_class.numel() == P && layer_class.device() == like.device() &&
                    (layer_class.scalar_type() == torch::kUInt8 || layer_class.scalar_type() == torch::kBool),
                "layer_class must be a uint8 / bool tensor of P elements on the device of the frame");
    p_cls = (const unsigned char*)(k_cls = layer_class.contiguous()).data_ptr();
  }
  torch::Tensor alpha_object = torch::empty({1, H, W}, like.options().dtype(torch::kFloat32));
  torch::Tensor workspace =
      torch::empty({(int64_t)grpg_object_alpha_workspace_bytes(W, H)}, like.options().dtype(torch::kByte));
  run("grpg_object_alpha_forward", [&](void* stream) {
    return grpg_object_alpha_forward((int)P, W, H, p_cls, reinterpret_cast<char*>(geomBuffer.data_ptr()),
                                     reinterpret_cast<char*>(binningBuffer.data_ptr()),
                                     reinterpret_cast<char*>(imageBuffer.data_ptr()), alpha_object.data_ptr<float>(),
                                     reinterpret_cast<char*>(workspace.data_ptr()), stream);
  });
  return std::make_tuple(alpha_object, workspace);
}

// (means3D [P,3], scales [P,3], rotations [P,4], opacity [P,1], shs [P,M,3]): what the reference's
// get_xyz / get_scaling / get_rotation / get_opacity / get_features return for the same models
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
Compose(GRPG_MODEL_PARAMS) {
  SegmentPack pk = pack_segments(GRPG_MODEL_ARGS);
  const torch::Tensor& like = xyz[0];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
  auto o = like.options().dtype(torch::kFloat32);
  torch::Tensor means = torch::empty({pk.P, 3}, o), scales = torch::empty({pk.P, 3}, o),
                rots = torch::empty({pk.P, 4}, o), opac = torch::empty({pk.P, 1}, o),
                shs = torch::empty({pk.P, pk.M, 3}, o);
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (int rc = pk.bind()) raise_abi_error("grpg_bind_device_poses", rc);
  const int rc = grpg_compose(pk.segs.data(), (int)pk.segs.size(), pk.M, means.data_ptr<float>(),
                              scales.data_ptr<float>(), rots.data_ptr<float>(), opac.data_ptr<float>(),
                              shs.data_ptr<float>(), (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_compose", rc);
  return std::make_tuple(means, scales, rots, opac, shs);
}

// ----------------------------------------------------------------------------------------------
// Sky cube map (additive; include/grpg_rasterizer.h: grpg_sky_composite / grpg_sky_backward).
// ray_matrix: CPU float tensor [3,3] = R^T K^-1.
// ----------------------------------------------------------------------------------------------
// ray_matrix [3,3] float32 = R^T K^-1, on the CPU or on the cube map's device (the latter costs no
// host read of the camera); mask (bool / uint8 [H,W]) and jitter (float32 [2,H,W]) are the train-mode
// extras of grpg_sky_composite_ex.
static const unsigned char* sky_mask_ptr(const c10::optional<torch::Tensor>& mask_opt, torch::Tensor& hold,
                                         const int height, const int width) {
  if (!mask_opt.has_value() || !mask_opt->defined()) return nullptr;
  TORCH_CHECK(mask_opt->is_cuda() && (mask_opt->scalar_type() == torch::kBool ||
                                      mask_opt->scalar_type() == torch::kUInt8) &&
                  mask_opt->numel() == (int64_t)height * width,
              "sky mask must be a bool / uint8 device tensor [H,W]");
  hold = mask_opt->contiguous();
  return (const unsigned char*)hold.data_ptr();
}
static const float* sky_jitter_ptr(const c10::optional<torch::Tensor>& jit_opt, torch::Tensor& hold,
                                   const int height, const int width) {
  if (!jit_opt.has_value() || !jit_opt->defined()) return nullptr;
  TORCH_CHECK(jit_opt->is_cuda() && jit_opt->scalar_type() == torch::kFloat32 &&
                  jit_opt->numel() == 2 * (int64_t)height * width,
              "sky jitter must be a float32 device tensor [2,H,W]");
  hold = jit_opt->contiguous();
  return hold.data_ptr<float>();
}
static void check_ray_matrix(const torch::Tensor& ray_matrix, const torch::Tensor& cube) {
  TORCH_CHECK(ray_matrix.scalar_type() == torch::kFloat32 && ray_matrix.numel() == 9 &&
                  (!ray_matrix.is_cuda() || ray_matrix.device() == cube.device()),
              "ray_matrix must be a float32 tensor [3,3] on the CPU or on the cube map's device");
}

std::tuple<torch::Tensor, torch::Tensor>
SkyComposite(const torch::Tensor& cube, const torch::Tensor& ray_matrix, const float fill,
             const bool clamp_out, const c10::optional<torch::Tensor>& rgb_opt,
             const c10::optional<torch::Tensor>& acc_opt, const int height, const int width,
             const bool want_sky, const c10::optional<torch::Tensor>& mask_opt,
             const c10::optional<torch::Tensor>& jitter_opt) {
  TORCH_CHECK(cube.is_cuda() && cube.scalar_type() == torch::kFloat32 && cube.dim() == 4 &&
                  cube.size(0) == 6 && cube.size(1) == cube.size(2) && cube.size(3) == 3,
              "sky cube map must be a float32 device tensor [6,res,res,3]");
  check_ray_matrix(ray_matrix, cube);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(cube.device());
  torch::Tensor cu = cube.contiguous(), rm = ray_matrix.contiguous(), rgb, acc, out, sky, mask, jit;
  const float* p_rgb = nullptr;
  const float* p_acc = nullptr;
  if (rgb_opt.has_value() && rgb_opt->defined()) {
    TORCH_CHECK(rgb_opt->is_cuda() && rgb_opt->scalar_type() == torch::kFloat32 && rgb_opt->dim() == 3 &&
                    rgb_opt->size(0) == 3 && rgb_opt->size(1) == height && rgb_opt->size(2) == width,
                "rgb must be a float32 device tensor [3,H,W]");
    rgb = rgb_opt->contiguous();
    p_rgb = rgb.data_ptr<float>();
    out = torch::empty_like(rgb);
  }
  if (acc_opt.has_value() && acc_opt->defined()) {
    TORCH_CHECK(acc_opt->is_cuda() && acc_opt->scalar_type() == torch::kFloat32 &&
                    acc_opt->numel() == (int64_t)height * width, "acc must be a float32 device tensor [1,H,W]");
    acc = acc_opt->contiguous();
    p_acc = acc.data_ptr<float>();
  }
  const unsigned char* p_mask = sky_mask_ptr(mask_opt, mask, height, width);
  const float* p_jit = sky_jitter_ptr(jitter_opt, jit, height, width);
  if (want_sky || !p_rgb) sky = torch::empty({3, height, width}, cu.options());
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int rc = grpg_sky_composite_ex(cu.data_ptr<float>(), (int)cu.size(1), rm.data_ptr<float>(),
                                       rm.is_cuda() ? 1 : 0, fill, clamp_out ? 1 : 0, width, height, p_rgb,
                                       p_acc, p_mask, p_jit, p_rgb ? out.data_ptr<float>() : nullptr,
                                       sky.defined() ? sky.data_ptr<float>() : nullptr, (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_sky_composite", rc);
  return std::make_tuple(out, sky);
}

std::tuple<torch::Tensor, torch::Tensor>
SkyBackward(const torch::Tensor& cube, const torch::Tensor& ray_matrix, const float fill,
            const c10::optional<torch::Tensor>& acc_opt, const torch::Tensor& grad_rgb,
            const c10::optional<torch::Tensor>& mask_opt, const c10::optional<torch::Tensor>& jitter_opt) {
  TORCH_CHECK(cube.is_cuda() && cube.scalar_type() == torch::kFloat32 && grad_rgb.is_cuda() &&
                  grad_rgb.scalar_type() == torch::kFloat32 && grad_rgb.dim() == 3 && grad_rgb.size(0) == 3,
              "cube and grad_rgb [3,H,W] must be float32 device tensors");
  check_ray_matrix(ray_matrix, cube);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(cube.device());
  const int H = grad_rgb.size(1), W = grad_rgb.size(2);
  torch::Tensor cu = cube.contiguous(), rm = ray_matrix.contiguous(), g = grad_rgb.contiguous(), acc, mask, jit;
  const float* p_acc = nullptr;
  if (acc_opt.has_value() && acc_opt->defined()) {
    TORCH_CHECK(acc_opt->is_cuda() && acc_opt->scalar_type() == torch::kFloat32 &&
                    acc_opt->numel() == (int64_t)H * W, "acc must be a float32 device tensor [1,H,W]");
    acc = acc_opt->contiguous();
    p_acc = acc.data_ptr<float>();
  }
  const unsigned char* p_mask = sky_mask_ptr(mask_opt, mask, H, W);
  const float* p_jit = sky_jitter_ptr(jitter_opt, jit, H, W);
  torch::Tensor grad_cube = torch::zeros_like(cu);
  torch::Tensor grad_acc = torch::empty({1, H, W}, cu.options());
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int rc = grpg_sky_backward_ex(cu.data_ptr<float>(), (int)cu.size(1), rm.data_ptr<float>(),
                                      rm.is_cuda() ? 1 : 0, fill, W, H, p_acc, p_mask, p_jit,
                                      g.data_ptr<float>(), grad_cube.data_ptr<float>(),
                                      grad_acc.data_ptr<float>(), (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_sky_backward", rc);
  return std::make_tuple(grad_cube, grad_acc);
}

// Parity/debug accessor (no reference counterpart): decode the private blobs of a
// forward call into the reference's intermediate arrays.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
DebugExport(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer,
            const torch::Tensor& imgBuffer, const int P, const int R, const int image_height,
            const int image_width) {
  TORCH_CHECK(geomBuffer.is_cuda(), "buffers must be device tensors");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(geomBuffer.device());
  const int gx = (image_width + GRPG_TILE_X - 1) / GRPG_TILE_X;
  const int gy = (image_height + GRPG_TILE_Y - 1) / GRPG_TILE_Y;
  auto o = geomBuffer.options();
  torch::Tensor keys = torch::zeros({R}, o.dtype(torch::kInt64));
  torch::Tensor plist = torch::zeros({R}, o.dtype(torch::kInt32));
  torch::Tensor ranges = torch::zeros({gx * gy, 2}, o.dtype(torch::kInt32));
  torch::Tensor ncontrib = torch::zeros({image_height, image_width}, o.dtype(torch::kInt32));
  torch::Tensor means2D = torch::zeros({P, 2}, o.dtype(torch::kFloat32));
  torch::Tensor depths = torch::zeros({P}, o.dtype(torch::kFloat32));
  torch::Tensor conic = torch::zeros({P, 4}, o.dtype(torch::kFloat32));
  torch::Tensor rgb = torch::zeros({P, 3}, o.dtype(torch::kFloat32));
  torch::Tensor tiles = torch::zeros({P}, o.dtype(torch::kInt32));
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int rc = grpg_debug_export(
      P, R, image_width, image_height, reinterpret_cast<const char*>(geomBuffer.data_ptr()),
      reinterpret_cast<const char*>(binningBuffer.data_ptr()),
      reinterpret_cast<const char*>(imgBuffer.data_ptr()),
      reinterpret_cast<uint64_t*>(keys.data_ptr<int64_t>()),
      reinterpret_cast<uint32_t*>(plist.data_ptr<int>()),
      reinterpret_cast<uint32_t*>(ranges.data_ptr<int>()),
      reinterpret_cast<uint32_t*>(ncontrib.data_ptr<int>()), means2D.data_ptr<float>(),
      depths.data_ptr<float>(), conic.data_ptr<float>(), rgb.data_ptr<float>(),
      reinterpret_cast<uint32_t*>(tiles.data_ptr<int>()), (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_debug_export", rc);
  return std::make_tuple(keys, plist, ranges, ncontrib, means2D, depths, conic, rgb, tiles);
}

// out: optional preallocated uint8 tensor of the same shape (e.g. a slot of the gather buffer), so
// that the packed frame is written in place instead of being copied there afterwards
torch::Tensor PackU8(const torch::Tensor& color, const c10::optional<torch::Tensor>& out_opt) {
  TORCH_CHECK(color.is_cuda() && color.scalar_type() == torch::kFloat32, "pack_u8: float32 device tensor");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(color.device());
  torch::Tensor src = color.contiguous();
  torch::Tensor out;
  if (out_opt.has_value() && out_opt->defined()) {
    out = *out_opt;
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kUInt8 && out.is_contiguous() &&
                    out.numel() == src.numel(), "pack_u8: out must be a contiguous uint8 device tensor of the same size");
  } else {
    out = torch::empty(src.sizes(), src.options().dtype(torch::kUInt8));
  }
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int rc = grpg_pack_rgb_u8(src.data_ptr<float>(), out.data_ptr<uint8_t>(), (size_t)src.numel(),
                                  (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_pack_rgb_u8", rc);
  return out;
}

// float [3,H,W] -> uint8 [H,W,3] (rgb8); truncate=true reproduces the simulator's astype(uint8)
torch::Tensor PackHWC(const torch::Tensor& color, const bool truncate) {
  TORCH_CHECK(color.is_cuda() && color.scalar_type() == torch::kFloat32 && color.dim() == 3 &&
                  color.size(0) == 3, "pack_hwc: float32 device tensor [3,H,W]");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(color.device());
  torch::Tensor src = color.contiguous();
  const int H = src.size(1), W = src.size(2);
  torch::Tensor out = torch::empty({H, W, 3}, src.options().dtype(torch::kUInt8));
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int rc = grpg_pack_rgb_u8_hwc(src.data_ptr<float>(), out.data_ptr<uint8_t>(), H, W,
                                      truncate ? 1 : 0, (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_pack_rgb_u8_hwc", rc);
  return out;
}

// ---- colour correction of the frame (gaussianrpg_amd/appearance.py; csrc/color_correction.hip) ----
namespace {
using OptTensor = c10::optional<torch::Tensor>;

bool given(const OptTensor& t) { return t.has_value() && t->defined(); }

// rgb: float32 device [3,H,W]; affine: float32 [3,4] on the same device (a view of the parameter is taken as it is);
// the sky inputs (cube, ray_matrix, acc) all or none, mask / jitter only with them.
struct ColorCorrectIn {
  torch::Tensor rgb, affine, cube, rm, acc, mask, jit;   // contiguous
  int H = 0, W = 0, res = 0, rm_dev = 0;
  const float *p_cube = nullptr, *p_rm = nullptr, *p_acc = nullptr, *p_jit = nullptr;
  const unsigned char* p_mask = nullptr;
};

ColorCorrectIn color_correct_args(const torch::Tensor& rgb, const torch::Tensor& affine, const OptTensor& cube,
                                  const OptTensor& ray_matrix, const OptTensor& acc, const OptTensor& mask,
                                  const OptTensor& jitter) {
  TORCH_CHECK(rgb.is_cuda(), "color_correct: the image must live on a ROCm/HIP device (no CPU path)");
  TORCH_CHECK(rgb.scalar_type() == torch::kFloat32 && rgb.dim() == 3 && rgb.size(0) == 3 && rgb.numel() > 0,
              "color_correct: the image must be a float32 tensor [3,H,W]");
  TORCH_CHECK(affine.device() == rgb.device() && affine.scalar_type() == torch::kFloat32 && affine.dim() == 2 &&
                  affine.size(0) == 3 && affine.size(1) == 4,
              "color_correct: affine must be a float32 tensor [3,4] on the image's device");
  ColorCorrectIn in;
  in.rgb = rgb.contiguous();
  in.affine = affine.contiguous();
  in.H = in.rgb.size(1);
  in.W = in.rgb.size(2);
  if (!given(cube)) {
    TORCH_CHECK(!given(ray_matrix) && !given(acc) && !given(mask) && !given(jitter),
                "color_correct: ray_matrix / acc / mask / jitter need the sky cube map");
    return in;
  }
  TORCH_CHECK(given(ray_matrix) && given(acc), "color_correct: the sky inputs (cube, ray_matrix, acc) go together");
  TORCH_CHECK(cube->device() == rgb.device() && cube->scalar_type() == torch::kFloat32 && cube->dim() == 4 &&
                  cube->size(0) == 6 && cube->size(1) == cube->size(2) && cube->size(3) == 3,
              "sky cube map must be a float32 device tensor [6,res,res,3]");
  check_ray_matrix(*ray_matrix, *cube);
  TORCH_CHECK(acc->device() == rgb.device() && acc->scalar_type() == torch::kFloat32 &&
                  acc->numel() == (int64_t)in.H * in.W, "acc must be a float32 device tensor [1,H,W]");
  in.cube = cube->contiguous();
  in.rm = ray_matrix->contiguous();
  in.acc = acc->contiguous();
  in.res = in.cube.size(1);
  in.rm_dev = in.rm.is_cuda() ? 1 : 0;
  in.p_cube = in.cube.data_ptr<float>();
  in.p_rm = in.rm.data_ptr<float>();
  in.p_acc = in.acc.data_ptr<float>();
  in.p_mask = sky_mask_ptr(mask, in.mask, in.H, in.W);
  in.p_jit = sky_jitter_ptr(jitter, in.jit, in.H, in.W);
  return in;
}
}  // namespace

// (planes [3,H,W] or undefined, rgb8 [H,W,3] or undefined).  out: optional preallocated uint8 [H,W,3] for the bytes.
std::tuple<torch::Tensor, torch::Tensor> ColorCorrect(
    const torch::Tensor& rgb, const torch::Tensor& affine, const bool clamp, const bool planes, const bool rgb8,
    const bool truncate, const OptTensor& out_opt, const OptTensor& cube, const OptTensor& ray_matrix,
    const double fill, const OptTensor& acc, const OptTensor& mask, const OptTensor& jitter) {
  const ColorCorrectIn in = color_correct_args(rgb, affine, cube, ray_matrix, acc, mask, jitter);
  TORCH_CHECK(planes || rgb8, "color_correct: ask for the float planes, the rgb8 frame, or both");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.rgb.device());
  torch::Tensor out_planes, out_rgb8;
  if (planes) out_planes = torch::empty_like(in.rgb);
  if (rgb8) {
    if (given(out_opt)) {
      out_rgb8 = *out_opt;
      TORCH_CHECK(out_rgb8.device() == in.rgb.device() && out_rgb8.scalar_type() == torch::kUInt8 &&
                      out_rgb8.is_contiguous() && out_rgb8.dim() == 3 && out_rgb8.size(0) == in.H &&
                      out_rgb8.size(1) == in.W && out_rgb8.size(2) == 3,
                  "color_correct: out must be a contiguous uint8 tensor [H,W,3] on the image's device");
    } else {
      out_rgb8 = torch::empty({in.H, in.W, 3}, in.rgb.options().dtype(torch::kUInt8));
    }
  }
  run("grpg_color_correct_forward", [&](void* stream) {
    return grpg_color_correct_forward(in.W, in.H, in.rgb.data_ptr<float>(), in.affine.data_ptr<float>(), in.p_cube,
                                      in.res, in.p_rm, in.rm_dev, (float)fill, in.p_acc, in.p_mask, in.p_jit,
                                      clamp ? 1 : 0, planes ? out_planes.data_ptr<float>() : nullptr,
                                      rgb8 ? out_rgb8.data_ptr<uint8_t>() : nullptr, truncate ? 1 : 0, stream);
  });
  return std::make_tuple(out_planes, out_rgb8);
}

// (grad_x [3,H,W] = A^T grad or undefined, grad_affine [3,4] or undefined)
std::tuple<torch::Tensor, torch::Tensor> ColorCorrectBackward(
    const torch::Tensor& rgb, const torch::Tensor& affine, const torch::Tensor& grad, const bool need_x,
    const bool need_affine, const OptTensor& cube, const OptTensor& ray_matrix, const double fill,
    const OptTensor& acc, const OptTensor& mask, const OptTensor& jitter) {
  const ColorCorrectIn in = color_correct_args(rgb, affine, cube, ray_matrix, acc, mask, jitter);
  TORCH_CHECK(grad.device() == in.rgb.device() && grad.scalar_type() == torch::kFloat32 &&
                  grad.sizes() == in.rgb.sizes(),
              "color_correct_backward: the gradient must be a float32 tensor [3,H,W] on the image's device");
  TORCH_CHECK(need_x || need_affine, "color_correct_backward: ask for the image gradient, the matrix gradient, or both");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.rgb.device());
  const torch::Tensor g = grad.contiguous();
  torch::Tensor grad_x, grad_affine, ws;
  if (need_x) grad_x = torch::empty_like(in.rgb);
  if (need_affine) {
    grad_affine = torch::empty({3, 4}, in.rgb.options());
    ws = torch::empty({(long long)grpg_color_correct_workspace_bytes(in.W, in.H)},
                      in.rgb.options().dtype(torch::kByte));
  }
  run("grpg_color_correct_backward", [&](void* stream) {
    return grpg_color_correct_backward(in.W, in.H, in.rgb.data_ptr<float>(), in.affine.data_ptr<float>(), in.p_cube,
                                       in.res, in.p_rm, in.rm_dev, (float)fill, in.p_acc, in.p_mask, in.p_jit,
                                       g.data_ptr<float>(), need_x ? grad_x.data_ptr<float>() : nullptr,
                                       need_affine ? grad_affine.data_ptr<float>() : nullptr,
                                       need_affine ? ws.data_ptr() : nullptr, stream);
  });
  return std::make_tuple(grad_x, grad_affine);
}

// ---- colour correction, use_mlp variant (gaussianrpg_amd/appearance.py ColorCorrectionMLP; csrc/color_mlp.hip) ----
namespace {
const int64_t kColorMlpShape[4][2] = {{64, 6}, {64, 64}, {64, 64}, {12, 64}};

// weights / biases: eight tensors each, network-major ([affine_trans layers 0..3], [affine_trans_sky layers 0..3]);
// taken in place: float32, contiguous, on one device
torch::Device color_mlp_check(const std::vector<torch::Tensor>& weights, const std::vector<torch::Tensor>& biases,
                              const char* what) {
  TORCH_CHECK(weights.size() == 8 && biases.size() == 8, what, ": eight weights and eight biases (two networks x four layers)");
  TORCH_CHECK(weights[0].is_cuda(), what, ": the parameters must live on a ROCm/HIP device (no CPU path)");
  const torch::Device dev = weights[0].device();
  for (int i = 0; i < 8; i++) {
    const int64_t* s = kColorMlpShape[i & 3];
    TORCH_CHECK(weights[i].device() == dev && weights[i].scalar_type() == torch::kFloat32 &&
                    weights[i].is_contiguous() && weights[i].dim() == 2 && weights[i].size(0) == s[0] &&
                    weights[i].size(1) == s[1],
                what, ": weight ", i, " must be a contiguous float32 tensor [", s[0], ",", s[1], "] on one device");
    TORCH_CHECK(biases[i].device() == dev && biases[i].scalar_type() == torch::kFloat32 && biases[i].is_contiguous() &&
                    biases[i].dim() == 1 && biases[i].size(0) == s[0],
                what, ": bias ", i, " must be a contiguous float32 tensor [", s[0], "] on one device");
  }
  return dev;
}

grpg_color_mlp_params color_mlp_params(const std::vector<torch::Tensor>& weights,
                                       const std::vector<torch::Tensor>& biases) {
  grpg_color_mlp_params p;
  for (int i = 0; i < 8; i++) {
    p.weight[i >> 2][i & 3] = weights[i].data_ptr<float>();
    p.bias[i >> 2][i & 3] = biases[i].data_ptr<float>();
  }
  return p;
}
}  // namespace

// (affine [T,2,3,4], x [T,6], reg [T] or undefined, hidden [T,2,3,64] or undefined)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> ColorMlpForward(
    const std::vector<torch::Tensor>& weights, const std::vector<torch::Tensor>& biases, const torch::Tensor& ego_pose,
    const torch::Tensor& extrinsic, const bool want_reg, const bool want_hidden) {
  const torch::Device dev = color_mlp_check(weights, biases, "color_mlp_forward");
  TORCH_CHECK(ego_pose.device() == dev && ego_pose.scalar_type() == torch::kFloat32 && ego_pose.dim() == 3 &&
                  ego_pose.size(0) >= 1 && ego_pose.size(0) <= (1 << 20) && ego_pose.size(1) == 4 &&
                  ego_pose.size(2) == 4,
              "color_mlp_forward: ego_pose must be a float32 tensor [T,4,4] (1 <= T <= 2^20) on the parameters' device");
  const int T = (int)ego_pose.size(0);
  TORCH_CHECK(extrinsic.device() == dev && extrinsic.scalar_type() == torch::kFloat32 && extrinsic.dim() == 3 &&
                  (extrinsic.size(0) == T || extrinsic.size(0) == 1) && extrinsic.size(1) == 4 &&
                  extrinsic.size(2) == 4,
              "color_mlp_forward: extrinsic must be a float32 tensor [T,4,4] or [1,4,4] on the parameters' device");
  const torch::Tensor ego = ego_pose.contiguous(), ext = extrinsic.contiguous();
  const int shared = (extrinsic.size(0) == 1 && T > 1) ? 1 : 0;
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  const auto opt = ego.options();
  torch::Tensor affine = torch::empty({T, 2, 3, 4}, opt), x = torch::empty({T, 6}, opt), reg, hidden;
  if (want_reg) reg = torch::empty({T}, opt);
  if (want_hidden) hidden = torch::empty({T, 2, 3, 64}, opt);
  const grpg_color_mlp_params p = color_mlp_params(weights, biases);
  run("grpg_color_mlp_forward", [&](void* stream) {
    return grpg_color_mlp_forward(&p, T, ego.data_ptr<float>(), ext.data_ptr<float>(), shared,
                                  affine.data_ptr<float>(), x.data_ptr<float>(),
                                  want_reg ? reg.data_ptr<float>() : nullptr,
                                  want_hidden ? hidden.data_ptr<float>() : nullptr, stream);
  });
  return std::make_tuple(affine, x, reg, hidden);
}

// (weight gradients x 8, bias gradients x 8), network-major like the parameters.  grad_affine [T,2,3,4] and / or
// grad_reg [T]; affine: the forward's output (read only with grad_reg).
std::tuple<std::vector<torch::Tensor>, std::vector<torch::Tensor>> ColorMlpBackward(
    const std::vector<torch::Tensor>& weights, const std::vector<torch::Tensor>& biases, const torch::Tensor& x,
    const torch::Tensor& hidden, const torch::Tensor& affine, const c10::optional<torch::Tensor>& grad_affine,
    const c10::optional<torch::Tensor>& grad_reg) {
  const torch::Device dev = color_mlp_check(weights, biases, "color_mlp_backward");
  TORCH_CHECK(x.device() == dev && x.scalar_type() == torch::kFloat32 && x.is_contiguous() && x.dim() == 2 &&
                  x.size(0) >= 1 && x.size(0) <= (1 << 20) && x.size(1) == 6,
              "color_mlp_backward: x must be the forward's contiguous float32 [T,6]");
  const int64_t T = x.size(0);
  const auto is = [&](const torch::Tensor& t, at::IntArrayRef shape) {
    return t.device() == dev && t.scalar_type() == torch::kFloat32 && t.sizes() == shape;
  };
  TORCH_CHECK(is(hidden, {T, 2, 3, 64}) && hidden.is_contiguous() && is(affine, {T, 2, 3, 4}) && affine.is_contiguous(),
              "color_mlp_backward: hidden [T,2,3,64] and affine [T,2,3,4] must be the forward's outputs");
  const bool has_ga = grad_affine.has_value() && grad_affine->defined();
  const bool has_gr = grad_reg.has_value() && grad_reg->defined();
  TORCH_CHECK(has_ga || has_gr, "color_mlp_backward: give grad_affine, grad_reg, or both");
  TORCH_CHECK(!has_ga || is(*grad_affine, {T, 2, 3, 4}), "color_mlp_backward: grad_affine must be float32 [T,2,3,4]");
  TORCH_CHECK(!has_gr || is(*grad_reg, {T}), "color_mlp_backward: grad_reg must be float32 [T]");
  torch::Tensor ga, gr;
  if (has_ga) ga = grad_affine->contiguous();
  if (has_gr) gr = grad_reg->contiguous();
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  std::vector<torch::Tensor> gw, gb;
  grpg_color_mlp_grads g;
  for (int i = 0; i < 8; i++) {
    gw.push_back(torch::empty_like(weights[i]));
    gb.push_back(torch::empty_like(biases[i]));
    g.weight[i >> 2][i & 3] = gw[i].data_ptr<float>();
    g.bias[i >> 2][i & 3] = gb[i].data_ptr<float>();
  }
  const grpg_color_mlp_params p = color_mlp_params(weights, biases);
  run("grpg_color_mlp_backward", [&](void* stream) {
    return grpg_color_mlp_backward(&p, (int)T, x.data_ptr<float>(), hidden.data_ptr<float>(),
                                   affine.data_ptr<float>(), has_ga ? ga.data_ptr<float>() : nullptr,
                                   has_gr ? gr.data_ptr<float>() : nullptr, &g, stream);
  });
  return std::make_tuple(gw, gb);
}

// ---- pose correction of the background (gaussianrpg_amd/pose_correction.py; csrc/pose_correction.hip) ----
namespace {
// xyz [N,3] and / or rotation [N,4] (float32, on a device, the same N); rot [4] / trans [3] float32 on that device (a
// view of the parameter is taken as it is).
struct PoseCorrectIn {
  torch::Tensor xyz, rotation, rot, trans;   // contiguous; xyz / rotation undefined when absent
  int N = 0;
  torch::Tensor any;                          // whichever input is there: device and options
};

PoseCorrectIn pose_correct_args(const OptTensor& xyz, const OptTensor& rotation, const torch::Tensor& rot,
                                const torch::Tensor& trans) {
  TORCH_CHECK(given(xyz) || given(rotation), "pose_correct: give xyz, rotation, or both");
  PoseCorrectIn in;
  in.any = given(xyz) ? *xyz : *rotation;
  TORCH_CHECK(in.any.is_cuda(), "pose_correct: the Gaussians must live on a ROCm/HIP device (no CPU path)");
  if (given(xyz)) {
    TORCH_CHECK(xyz->scalar_type() == torch::kFloat32 && xyz->dim() == 2 && xyz->size(1) == 3,
                "pose_correct: xyz must be a float32 tensor [N,3]");
    in.xyz = xyz->contiguous();
  }
  if (given(rotation)) {
    TORCH_CHECK(rotation->device() == in.any.device() && rotation->scalar_type() == torch::kFloat32 &&
                    rotation->dim() == 2 && rotation->size(1) == 4,
                "pose_correct: rotation must be a float32 tensor [N,4] on the device of xyz");
    TORCH_CHECK(!given(xyz) || rotation->size(0) == xyz->size(0), "pose_correct: xyz and rotation disagree on N");
    in.rotation = rotation->contiguous();
  }
  TORCH_CHECK(in.any.size(0) <= INT_MAX, "pose_correct: too many rows");
  in.N = (int)in.any.size(0);
  TORCH_CHECK(rot.device() == in.any.device() && rot.scalar_type() == torch::kFloat32 && rot.numel() == 4 &&
                  trans.device() == in.any.device() && trans.scalar_type() == torch::kFloat32 && trans.numel() == 3,
              "pose_correct: rot [4] and trans [3] must be float32 tensors on the Gaussians' device");
  in.rot = rot.contiguous();
  in.trans = trans.contiguous();
  return in;
}

const float* ptr_or_null(const torch::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
float* mut_ptr_or_null(torch::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
}  // namespace

// (xyz' [N,3] or undefined, rotation' [N,4] or undefined)
std::tuple<torch::Tensor, torch::Tensor> PoseCorrect(const OptTensor& xyz, const OptTensor& rotation,
                                                     const torch::Tensor& rot, const torch::Tensor& trans) {
  const PoseCorrectIn in = pose_correct_args(xyz, rotation, rot, trans);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.any.device());
  torch::Tensor out_xyz, out_rotation;
  if (in.xyz.defined()) out_xyz = torch::empty_like(in.xyz);
  if (in.rotation.defined()) out_rotation = torch::empty_like(in.rotation);
  if (in.N == 0) return std::make_tuple(out_xyz, out_rotation);   // nothing to launch; empty tensors have no address
  run("grpg_pose_correct_forward", [&](void* stream) {
    return grpg_pose_correct_forward(in.N, ptr_or_null(in.xyz), ptr_or_null(in.rotation), in.rot.data_ptr<float>(),
                                     in.trans.data_ptr<float>(), mut_ptr_or_null(out_xyz),
                                     mut_ptr_or_null(out_rotation), stream);
  });
  return std::make_tuple(out_xyz, out_rotation);
}

// (g_xyz [N,3], g_rotation [N,4], g_rot [4], g_trans [3]); each undefined when not asked for.  grad_xyz /
// grad_rotation: the upstream gradients of the outputs the forward gave (an absent one counts as zero).
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> PoseCorrectBackward(
    const OptTensor& xyz, const OptTensor& rotation, const torch::Tensor& rot, const torch::Tensor& trans,
    const OptTensor& grad_xyz, const OptTensor& grad_rotation, const bool need_xyz, const bool need_rotation,
    const bool need_rot, const bool need_trans) {
  TORCH_CHECK(given(grad_xyz) || given(grad_rotation), "pose_correct_backward: give at least one upstream gradient");
  TORCH_CHECK((!given(grad_xyz) || given(xyz)) && (!given(grad_rotation) || given(rotation)),
              "pose_correct_backward: an upstream gradient needs its forward input");
  const PoseCorrectIn in = pose_correct_args(given(grad_xyz) ? xyz : OptTensor(),
                                             given(grad_rotation) ? rotation : OptTensor(), rot, trans);
  TORCH_CHECK(need_xyz || need_rotation || need_rot || need_trans, "pose_correct_backward: ask for a gradient");
  TORCH_CHECK((!need_xyz || given(grad_xyz)) && (!need_rotation || given(grad_rotation)),
              "pose_correct_backward: an input gradient needs its upstream gradient");
  torch::Tensor gox, gor;
  if (given(grad_xyz)) {
    TORCH_CHECK(grad_xyz->device() == in.any.device() && grad_xyz->scalar_type() == torch::kFloat32 &&
                    grad_xyz->sizes() == in.xyz.sizes(),
                "pose_correct_backward: grad_xyz must be a float32 tensor [N,3] on the Gaussians' device");
    gox = grad_xyz->contiguous();
  }
  if (given(grad_rotation)) {
    TORCH_CHECK(grad_rotation->device() == in.any.device() && grad_rotation->scalar_type() == torch::kFloat32 &&
                    grad_rotation->sizes() == in.rotation.sizes(),
                "pose_correct_backward: grad_rotation must be a float32 tensor [N,4] on the Gaussians' device");
    gor = grad_rotation->contiguous();
  }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.any.device());
  torch::Tensor g_xyz, g_rotation, g_rot, g_trans, ws;
  if (need_xyz) g_xyz = torch::empty_like(in.xyz);
  if (need_rotation) g_rotation = torch::empty_like(in.rotation);
  if (need_rot) g_rot = torch::empty({4}, in.any.options());
  if (need_trans) g_trans = torch::empty({3}, in.any.options());
  if (in.N == 0) {   // sums over no rows
    if (need_rot) g_rot.zero_();
    if (need_trans) g_trans.zero_();
    return std::make_tuple(g_xyz, g_rotation, g_rot, g_trans);
  }
  if (need_rot || need_trans)
    ws = torch::empty({(long long)grpg_pose_correct_workspace_bytes(in.N)}, in.any.options().dtype(torch::kByte));
  run("grpg_pose_correct_backward", [&](void* stream) {
    return grpg_pose_correct_backward(in.N, ptr_or_null(in.xyz), ptr_or_null(in.rotation), in.rot.data_ptr<float>(),
                                      ptr_or_null(gox), ptr_or_null(gor), mut_ptr_or_null(g_xyz),
                                      mut_ptr_or_null(g_rotation), mut_ptr_or_null(g_rot), mut_ptr_or_null(g_trans),
                                      ws.defined() ? ws.data_ptr() : nullptr, stream);
  });
  return std::make_tuple(g_xyz, g_rotation, g_rot, g_trans);
}

namespace {
void pose_rows_params(const torch::Tensor& corr_rots, const torch::Tensor& corr_trans, const int64_t id) {
  TORCH_CHECK(corr_rots.is_cuda(), "pose_rows: the correction parameters must live on a ROCm/HIP device");
  TORCH_CHECK(corr_rots.scalar_type() == torch::kFloat32 && corr_rots.dim() == 2 && corr_rots.size(1) == 4 &&
                  corr_trans.device() == corr_rots.device() && corr_trans.scalar_type() == torch::kFloat32 &&
                  corr_trans.dim() == 2 && corr_trans.size(1) == 3 && corr_trans.size(0) == corr_rots.size(0),
              "pose_rows: the correction parameters must be float32 tensors [n,4] and [n,3] on one device");
  TORCH_CHECK(id >= 0 && id < corr_rots.size(0), "pose_rows: id ", id, " is not one of the ", corr_rots.size(0),
              " correction rows");
}
}  // namespace

// (rot' [A+1,4], trans' [A+1,3]): the actors' rows, then the raw correction row id
std::tuple<torch::Tensor, torch::Tensor> PoseRowsForward(const torch::Tensor& rot, const torch::Tensor& trans,
                                                         const torch::Tensor& corr_rots,
                                                         const torch::Tensor& corr_trans, const int64_t id) {
  pose_rows_params(corr_rots, corr_trans, id);
  TORCH_CHECK(rot.device() == corr_rots.device() && rot.scalar_type() == torch::kFloat32 && rot.dim() == 2 &&
                  rot.size(1) == 4 && trans.device() == corr_rots.device() &&
                  trans.scalar_type() == torch::kFloat32 && trans.dim() == 2 && trans.size(1) == 3 &&
                  trans.size(0) == rot.size(0),
              "pose_rows: the actors' rows must be float32 tensors [A,4] and [A,3] on the parameters' device");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(corr_rots.device());
  const int A = (int)rot.size(0);
  const torch::Tensor r = rot.contiguous(), t = trans.contiguous(), cr = corr_rots.contiguous(),
                      ct = corr_trans.contiguous();
  torch::Tensor out_rot = torch::empty({A + 1, 4}, cr.options()), out_trans = torch::empty({A + 1, 3}, cr.options());
  run("grpg_pose_rows_forward", [&](void* stream) {
    return grpg_pose_rows_forward(A, A ? r.data_ptr<float>() : nullptr, A ? t.data_ptr<float>() : nullptr,
                                  (int)cr.size(0), cr.data_ptr<float>(), ct.data_ptr<float>(), (int)id,
                                  out_rot.data_ptr<float>(), out_trans.data_ptr<float>(), stream);
  });
  return std::make_tuple(out_rot, out_trans);
}

// (g_corr_rots [n,4], g_corr_trans [n,3]) from the table's gradient [A+1,4] / [A+1,3]
std::tuple<torch::Tensor, torch::Tensor> PoseRowsBackward(const torch::Tensor& grad_rot, const torch::Tensor& grad_trans,
                                                          const int64_t n, const int64_t id) {
  TORCH_CHECK(grad_rot.is_cuda() && grad_rot.scalar_type() == torch::kFloat32 && grad_rot.dim() == 2 &&
                  grad_rot.size(1) == 4 && grad_rot.size(0) >= 1 && grad_trans.device() == grad_rot.device() &&
                  grad_trans.scalar_type() == torch::kFloat32 && grad_trans.dim() == 2 && grad_trans.size(1) == 3 &&
                  grad_trans.size(0) == grad_rot.size(0),
              "pose_rows_backward: the gradients must be float32 device tensors [A+1,4] and [A+1,3]");
  TORCH_CHECK(n > 0 && n <= INT_MAX && id >= 0 && id < n, "pose_rows_backward: id must be one of the n rows");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(grad_rot.device());
  const torch::Tensor gr = grad_rot.contiguous(), gt = grad_trans.contiguous();
  torch::Tensor g_rots = torch::empty({n, 4}, gr.options()), g_trans = torch::empty({n, 3}, gr.options());
  run("grpg_pose_rows_backward", [&](void* stream) {
    return grpg_pose_rows_backward((int)gr.size(0) - 1, (int)n, (int)id, gr.data_ptr<float>(), gt.data_ptr<float>(),
                                   g_rots.data_ptr<float>(), g_trans.data_ptr<float>(), stream);
  });
  return std::make_tuple(g_rots, g_trans);
}

// ---- frame -> detector input (gaussianrpg_amd/perception.py; csrc/letterbox.hip) ----

// letterbox()'s arithmetic (utils/augmentations.py:121-151); host only.
// Returns [new_h, new_w, top, bottom, left, right, h, w].
std::vector<int> LetterboxGeometry(const int height, const int width, const int new_h_req, const int new_w_req,
                                   const bool auto_pad, const bool scale_fill, const bool scaleup, const int stride) {
  std::vector<int> g(8, 0);
  const int rc = grpg_letterbox_geometry(height, width, new_h_req, new_w_req, auto_pad, scale_fill, scaleup, stride,
                                         g.data());
  if (rc != GRPG_OK) raise_abi_error("grpg_letterbox_geometry", rc);
  return g;
}

// (x_table int32 [new_w,2], y_table int32 [new_h,2]) on the host; the entry format is in the C header.
std::tuple<torch::Tensor, torch::Tensor> LetterboxTables(const int height, const int width, const int new_h,
                                                         const int new_w) {
  TORCH_CHECK(height > 0 && width > 0 && new_h > 0 && new_w > 0, "letterbox_tables: sizes must be positive");
  torch::Tensor xt = torch::empty({new_w, 2}, torch::kInt32), yt = torch::empty({new_h, 2}, torch::kInt32);
  const int rc = grpg_letterbox_tables(height, width, new_h, new_w, xt.data_ptr<int>(), yt.data_ptr<int>());
  if (rc != GRPG_OK) raise_abi_error("grpg_letterbox_tables", rc);
  return std::make_tuple(xt, yt);
}

namespace {
// What the two letterbox bindings share.  The checks run in this order: the frame's dtype and shape (by the
// caller), geometry, out's dtype / shape / layout, then the devices -- so a host tensor is told "no CPU path" only
// when everything else about the call is right.
struct LetterboxCall {
  torch::Tensor out, xt, yt;
  const int *p_xt = nullptr, *p_yt = nullptr;
  bool half;

  LetterboxCall(const torch::Tensor& frame, const int H, const int W, const std::vector<int>& g,
                const c10::optional<torch::Tensor>& x_table, const c10::optional<torch::Tensor>& y_table,
                const c10::optional<torch::Tensor>& out_opt, const bool out_half) : half(out_half) {
    TORCH_CHECK(g.size() == 8, "letterbox: geometry must hold 8 ints (new_h, new_w, top, bottom, left, right, h, w)");
    TORCH_CHECK(g[6] > 0 && g[7] > 0, "letterbox: geometry gives an empty output");
    const int64_t h = g[6], w = g[7];
    const auto dtype = half ? torch::kFloat16 : torch::kFloat32;
    const bool given = out_opt.has_value() && out_opt->defined();
    if (given) {
      const torch::Tensor& o = *out_opt;
      TORCH_CHECK(o.scalar_type() == dtype, "letterbox: out must be ", half ? "float16" : "float32", " (got ",
                  o.scalar_type(), ")");
      const bool shape3 = o.dim() == 3 && o.size(0) == 3 && o.size(1) == h && o.size(2) == w;
      const bool shape4 = o.dim() == 4 && o.size(0) == 1 && o.size(1) == 3 && o.size(2) == h && o.size(3) == w;
      TORCH_CHECK(shape3 || shape4, "letterbox: out must be [3,", h, ",", w, "] or [1,3,", h, ",", w, "] (got ",
                  o.sizes(), ")");
      TORCH_CHECK(o.is_contiguous(), "letterbox: out must be contiguous");
    }
    TORCH_CHECK(frame.is_contiguous(), "letterbox: frame must be contiguous");
    TORCH_CHECK(frame.is_cuda(), "letterbox: frame must live on a ROCm/HIP device (torch device 'cuda'); "
                                 "this op has no CPU path");
    if (given) {
      TORCH_CHECK(out_opt->device() == frame.device(), "letterbox: out must be on ", frame.device(), " (got ",
                  out_opt->device(), ")");
      out = *out_opt;
    } else {
      out = torch::empty({1, 3, h, w}, frame.options().dtype(dtype));
    }
    if (g[0] != H || g[1] != W) {   // a resize: the tables are needed
      TORCH_CHECK(x_table.has_value() && x_table->defined() && y_table.has_value() && y_table->defined(),
                  "letterbox: x_table and y_table are needed when the resized size differs from the frame's");
      p_xt = table(*x_table, g[1], frame, "x_table", xt);
      p_yt = table(*y_table, g[0], frame, "y_table", yt);
    }
  }

  static const int* table(const torch::Tensor& t, const int64_t n, const torch::Tensor& frame, const char* name,
                          torch::Tensor& keep) {
    TORCH_CHECK(t.scalar_type() == torch::kInt32 && t.dim() == 2 && t.size(0) == n && t.size(1) == 2 &&
                    t.is_contiguous(), "letterbox: ", name, " must be a contiguous int32 [", n, ",2] tensor");
    TORCH_CHECK(t.device() == frame.device(), "letterbox: ", name, " must be on ", frame.device(), " (got ",
                t.device(), ")");
    keep = t;
    return t.data_ptr<int>();
  }
};
}  // namespace

// uint8 [H,W,3] device frame -> [1,3,h,w] (or `out`, returned as given)
torch::Tensor LetterboxRgb8(const torch::Tensor& frame, const std::vector<int>& geometry,
                            const c10::optional<torch::Tensor>& x_table, const c10::optional<torch::Tensor>& y_table,
                            const bool reverse_channels, const c10::optional<torch::Tensor>& out, const bool half) {
  TORCH_CHECK(frame.scalar_type() == torch::kUInt8, "letterbox_rgb8: frame must be uint8 (got ", frame.scalar_type(),
              ")");
  TORCH_CHECK(frame.dim() == 3 && frame.size(2) == 3 && frame.size(0) > 0 && frame.size(1) > 0,
              "letterbox_rgb8: frame must be [H,W,3] (got ", frame.sizes(), ")");
  const int H = frame.size(0), W = frame.size(1);
  LetterboxCall c(frame, H, W, geometry, x_table, y_table, out, half);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(frame.device());
  run("grpg_letterbox_rgb8", [&](void* stream) {
    return grpg_letterbox_rgb8(frame.data_ptr<uint8_t>(), H, W, geometry.data(), c.p_xt, c.p_yt, reverse_channels,
                               c.out.data_ptr(), half, stream);
  });
  return c.out;
}

// float32 [3,H,W] device planes -> the same, quantised on load as pack_hwc does
torch::Tensor LetterboxPlanes(const torch::Tensor& frame, const std::vector<int>& geometry,
                              const c10::optional<torch::Tensor>& x_table, const c10::optional<torch::Tensor>& y_table,
                              const bool reverse_channels, const bool truncate,
                              const c10::optional<torch::Tensor>& out, const bool half) {
  TORCH_CHECK(frame.scalar_type() == torch::kFloat32, "letterbox_planes: frame must be float32 (got ",
              frame.scalar_type(), ")");
  TORCH_CHECK(frame.dim() == 3 && frame.size(0) == 3 && frame.size(1) > 0 && frame.size(2) > 0,
              "letterbox_planes: frame must be [3,H,W] (got ", frame.sizes(), ")");
  const int H = frame.size(1), W = frame.size(2);
  LetterboxCall c(frame, H, W, geometry, x_table, y_table, out, half);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(frame.device());
  run("grpg_letterbox_planes", [&](void* stream) {
    return grpg_letterbox_planes(frame.data_ptr<float>(), H, W, geometry.data(), c.p_xt, c.p_yt, reverse_channels,
                                 truncate, c.out.data_ptr(), half, stream);
  });
  return c.out;
}

// ---- detector output -> detections (gaussianrpg_amd/perception.py; csrc/nms.hip) ----

// prediction float32 [bs,N,5+nc] on the device -> (det float32 [bs,max_det,6], count int32 [bs]), both written in
// full, no host wait.  class_allow: uint8 [nc] on the device or None; frame_map: () or (h, w, H, W, pad_x, pad_y);
// det_out / count_out: preallocated results, returned as given.
std::tuple<torch::Tensor, torch::Tensor> NmsDetections(const torch::Tensor& prediction, const double conf_thres,
                                                       const double iou_thres,
                                                       const c10::optional<torch::Tensor>& class_allow,
                                                       const bool agnostic, const int max_det, const int max_nms,
                                                       const double max_wh, const std::vector<double>& frame_map,
                                                       const c10::optional<torch::Tensor>& det_out,
                                                       const c10::optional<torch::Tensor>& count_out) {
  TORCH_CHECK(prediction.scalar_type() == torch::kFloat32, "nms_detections: prediction must be float32 (got ",
              prediction.scalar_type(), ")");
  TORCH_CHECK(prediction.dim() == 3 && prediction.size(0) > 0 && prediction.size(1) > 0 && prediction.size(2) >= 6,
              "nms_detections: prediction must be [bs,N,5+nc] with nc >= 1 (got ", prediction.sizes(), ")");
  TORCH_CHECK(prediction.is_contiguous(), "nms_detections: prediction must be contiguous");
  const int64_t bs = prediction.size(0), N = prediction.size(1), nc = prediction.size(2) - 5;
  TORCH_CHECK(bs * N < (int64_t(1) << 31), "nms_detections: bs * N must be below 2^31");
  TORCH_CHECK(conf_thres >= 0.0 && conf_thres <= 1.0 && iou_thres >= 0.0 && iou_thres <= 1.0,
              "nms_detections: conf_thres and iou_thres must lie in [0, 1]");
  TORCH_CHECK(max_det >= 1 && max_det <= 1024, "nms_detections: max_det must lie in [1, 1024] (got ", max_det, ")");
  TORCH_CHECK(max_nms >= 1, "nms_detections: max_nms must be positive");
  TORCH_CHECK(frame_map.empty() || frame_map.size() == 6,
              "nms_detections: frame_map must be empty or (h, w, H, W, pad_x, pad_y)");
  const bool det_given = det_out.has_value() && det_out->defined();
  const bool count_given = count_out.has_value() && count_out->defined();
  if (det_given)
    TORCH_CHECK(det_out->scalar_type() == torch::kFloat32 && det_out->dim() == 3 && det_out->size(0) == bs &&
                    det_out->size(1) == max_det && det_out->size(2) == 6 && det_out->is_contiguous(),
                "nms_detections: out det must be a contiguous float32 [", bs, ",", max_det, ",6] tensor");
  if (count_given)
    TORCH_CHECK(count_out->scalar_type() == torch::kInt32 && count_out->dim() == 1 && count_out->size(0) == bs &&
                    count_out->is_contiguous(),
                "nms_detections: out count must be a contiguous int32 [", bs, "] tensor");
  TORCH_CHECK(prediction.is_cuda(), "nms_detections: prediction must live on a ROCm/HIP device (torch device "
                                    "'cuda'); this op has no CPU path");
  const unsigned char* allow = nullptr;
  if (class_allow.has_value() && class_allow->defined()) {
    const torch::Tensor& t = *class_allow;
    TORCH_CHECK(t.scalar_type() == torch::kUInt8 && t.dim() == 1 && t.size(0) == nc && t.is_contiguous() &&
                    t.device() == prediction.device(),
                "nms_detections: class_allow must be a contiguous uint8 [", nc, "] tensor on ", prediction.device());
    allow = t.data_ptr<uint8_t>();
  }
  if (det_given) TORCH_CHECK(det_out->device() == prediction.device(), "nms_detections: out det must be on ",
                             prediction.device());
  if (count_given) TORCH_CHECK(count_out->device() == prediction.device(), "nms_detections: out count must be on ",
                               prediction.device());
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(prediction.device());
  torch::Tensor det = det_given ? *det_out : torch::empty({bs, max_det, 6}, prediction.options());
  torch::Tensor count = count_given ? *count_out : torch::empty({bs}, prediction.options().dtype(torch::kInt32));
  const size_t bytes = grpg_nms_workspace_bytes((int)bs, (int)N);
  torch::Tensor ws = torch::empty({(int64_t)bytes}, prediction.options().dtype(torch::kByte));
  run("grpg_nms_detections", [&](void* stream) {
    return grpg_nms_detections(prediction.data_ptr<float>(), (int)bs, (int)N, (int)nc, (float)conf_thres,
                               (float)iou_thres, allow, agnostic, max_det, max_nms, (float)max_wh,
                               frame_map.empty() ? nullptr : frame_map.data(), ws.data_ptr(), bytes,
                               det.data_ptr<float>(), count.data_ptr<int>(), stream);
  });
  return std::make_tuple(det, count);
}

// ---- detector head -> prediction / detections (gaussianrpg_amd/perception.py; csrc/nms.hip) ----

namespace {
// heads: the nl conv outputs float32 [bs, na*(5+nc), ny, nx]; anchor_grid: nl*na*2 pixels; stride: nl.  Everything is
// checked here, before the device is needed.
struct DetectCall {
  grpg_detect_geometry geom;
  std::vector<const float*> ptrs;
  int64_t bs = 0, N = 0;

  DetectCall(const char* what, const std::vector<torch::Tensor>& heads, const std::vector<double>& anchor_grid,
             const std::vector<double>& stride, const int64_t na, const int64_t nc) {
    const int64_t nl = (int64_t)stride.size();
    TORCH_CHECK(nl >= 1 && nl <= GRPG_DETECT_MAX_LEVELS && na >= 1 && nl * na <= GRPG_DETECT_MAX_ANCHORS,
                what, ": the geometry needs 1 <= nl <= 4, na >= 1 and nl * na <= 16 (got nl ", nl, ", na ", na, ")");
    TORCH_CHECK(nc >= 1, what, ": nc must be positive");
    TORCH_CHECK(nc < (int64_t(1) << 31) && na * (5 + nc) < (int64_t(1) << 31), what, ": na * (5 + nc) must be below 2^31");
    TORCH_CHECK((int64_t)anchor_grid.size() == nl * na * 2, what, ": anchor_grid must hold nl * na * 2 values");
    TORCH_CHECK((int64_t)heads.size() == nl, what, ": ", nl, " heads expected, one per level (got ", heads.size(), ")");
    geom = grpg_detect_geometry{};
    geom.nl = (int)nl; geom.na = (int)na; geom.nc = (int)nc;
    for (int64_t i = 0; i < nl * na * 2; i++) geom.anchor_grid[i / 2][i % 2] = (float)anchor_grid[i];
    for (int64_t l = 0; l < nl; l++) {
      const torch::Tensor& h = heads[l];
      TORCH_CHECK(h.scalar_type() == torch::kFloat32, what, ": head ", l, " must be float32 (got ", h.scalar_type(), ")");
      TORCH_CHECK(h.dim() == 4 && h.size(0) >= 1 && h.size(2) >= 1 && h.size(3) >= 1 && h.size(1) == na * (5 + nc),
                  what, ": head ", l, " must be [bs, na*(5+nc) = ", na * (5 + nc), ", ny, nx] (got ", h.sizes(), ")");
      TORCH_CHECK(h.is_contiguous(), what, ": head ", l, " must be contiguous");
      TORCH_CHECK(h.size(2) < (int64_t(1) << 31) && h.size(3) < (int64_t(1) << 31), what, ": bs * N must be below 2^31");
      if (l == 0) bs = h.size(0);
      TORCH_CHECK(h.size(0) == bs, what, ": every head must have the same bs (head 0 has ", bs, ", head ", l, " has ",
                  h.size(0), ")");
      TORCH_CHECK(h.device() == heads[0].device(), what, ": every head must be on ", heads[0].device());
      geom.ny[l] = (int)h.size(2); geom.nx[l] = (int)h.size(3);
      geom.stride[l] = (float)stride[l];
      N += na * h.size(2) * h.size(3);
      TORCH_CHECK(bs * N < (int64_t(1) << 31), what, ": bs * N must be below 2^31");
    }
    TORCH_CHECK(heads[0].is_cuda(), what, ": the heads must live on a ROCm/HIP device (torch device 'cuda'); this op "
                                          "has no CPU path");
    for (const torch::Tensor& h : heads) ptrs.push_back(h.data_ptr<float>());
  }
};
}  // namespace

torch::Tensor DetectDecode(const std::vector<torch::Tensor>& heads, const std::vector<double>& anchor_grid,
                           const std::vector<double>& stride, const int64_t na, const int64_t nc,
                           const c10::optional<torch::Tensor>& out) {
  DetectCall c("detect_decode", heads, anchor_grid, stride, na, nc);
  const bool given = out.has_value() && out->defined();
  if (given)
    TORCH_CHECK(out->scalar_type() == torch::kFloat32 && out->dim() == 3 && out->size(0) == c.bs && out->size(1) == c.N &&
                    out->size(2) == 5 + nc && out->is_contiguous() && out->device() == heads[0].device(),
                "detect_decode: out must be a contiguous float32 [", c.bs, ",", c.N, ",", 5 + nc, "] tensor on ",
                heads[0].device());
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(heads[0].device());
  torch::Tensor pred = given ? *out : torch::empty({c.bs, c.N, 5 + nc}, heads[0].options());
  run("grpg_detect_decode", [&](void* stream) {
    return grpg_detect_decode(c.ptrs.data(), &c.geom, (int)c.bs, pred.data_ptr<float>(), stream);
  });
  return pred;
}

std::tuple<torch::Tensor, torch::Tensor> DetectDetections(
    const std::vector<torch::Tensor>& heads, const std::vector<double>& anchor_grid, const std::vector<double>& stride,
    const int64_t na, const int64_t nc, const double conf_thres, const double iou_thres,
    const c10::optional<torch::Tensor>& class_allow, const bool agnostic, const int max_det, const int max_nms,
    const double max_wh, const std::vector<double>& frame_map, const c10::optional<torch::Tensor>& det_out,
    const c10::optional<torch::Tensor>& count_out) {
  DetectCall c("detect_detections", heads, anchor_grid, stride, na, nc);
  const int64_t bs = c.bs;
  const torch::Device device = heads[0].device();
  TORCH_CHECK(conf_thres >= 0.0 && conf_thres <= 1.0 && iou_thres >= 0.0 && iou_thres <= 1.0,
              "detect_detections: conf_thres and iou_thres must lie in [0, 1]");
  TORCH_CHECK(max_det >= 1 && max_det <= 1024, "detect_detections: max_det must lie in [1, 1024] (got ", max_det, ")");
  TORCH_CHECK(max_nms >= 1, "detect_detections: max_nms must be positive");
  TORCH_CHECK(frame_map.empty() || frame_map.size() == 6,
              "detect_detections: frame_map must be empty or (h, w, H, W, pad_x, pad_y)");
  const bool det_given = det_out.has_value() && det_out->defined();
  const bool count_given = count_out.has_value() && count_out->defined();
  if (det_given)
    TORCH_CHECK(det_out->scalar_type() == torch::kFloat32 && det_out->dim() == 3 && det_out->size(0) == bs &&
                    det_out->size(1) == max_det && det_out->size(2) == 6 && det_out->is_contiguous() &&
                    det_out->device() == device,
                "detect_detections: out det must be a contiguous float32 [", bs, ",", max_det, ",6] tensor on ", device);
  if (count_given)
    TORCH_CHECK(count_out->scalar_type() == torch::kInt32 && count_out->dim() == 1 && count_out->size(0) == bs &&
                    count_out->is_contiguous() && count_out->device() == device,
                "detect_detections: out count must be a contiguous int32 [", bs, "] tensor on ", device);
  const unsigned char* allow = nullptr;
  if (class_allow.has_value() && class_allow->defined()) {
    const torch::Tensor& t = *class_allow;
    TORCH_CHECK(t.scalar_type() == torch::kUInt8 && t.dim() == 1 && t.size(0) == nc && t.is_contiguous() &&
                    t.device() == device,
                "detect_detections: class_allow must be a contiguous uint8 [", nc, "] tensor on ", device);
    allow = t.data_ptr<uint8_t>();
  }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  torch::Tensor det = det_given ? *det_out : torch::empty({bs, max_det, 6}, heads[0].options());
  torch::Tensor count = count_given ? *count_out : torch::empty({bs}, heads[0].options().dtype(torch::kInt32));
  const size_t bytes = grpg_detect_workspace_bytes((int)bs, (int)c.N);
  torch::Tensor ws = torch::empty({(int64_t)bytes}, heads[0].options().dtype(torch::kByte));
  run("grpg_detect_detections", [&](void* stream) {
    return grpg_detect_detections(c.ptrs.data(), &c.geom, (int)bs, (float)conf_thres, (float)iou_thres, allow, agnostic,
                                  max_det, max_nms, (float)max_wh, frame_map.empty() ? nullptr : frame_map.data(),
                                  ws.data_ptr(), bytes, det.data_ptr<float>(), count.data_ptr<int>(), stream);
  });
  return std::make_tuple(det, count);
}

// ---- the detector's network (gaussianrpg_amd/detector.py; csrc/detector.hip) ----

// float32 [c_out, c_in, k, k] weight and [c_out] bias on the device -> the packed buffer the convolution streams.
torch::Tensor DetectorPackWeights(const torch::Tensor& weight, const torch::Tensor& bias) {
  TORCH_CHECK(weight.scalar_type() == torch::kFloat32 && bias.scalar_type() == torch::kFloat32,
              "detector_pack_weights: weight and bias must be float32");
  TORCH_CHECK(weight.dim() == 4 && weight.size(2) == weight.size(3) && bias.dim() == 1 && bias.size(0) == weight.size(0) &&
                  weight.is_contiguous() && bias.is_contiguous(),
              "detector_pack_weights: weight must be a contiguous [c_out, c_in, k, k] and bias [c_out] (got ",
              weight.sizes(), " and ", bias.sizes(), ")");
  TORCH_CHECK(weight.is_cuda() && bias.device() == weight.device(),
              "detector_pack_weights: weight and bias must live on one ROCm/HIP device (torch device 'cuda'); this op "
              "has no CPU path");
  TORCH_CHECK(weight.size(0) < (int64_t(1) << 24) && weight.size(1) < (int64_t(1) << 20), "detector_pack_weights: too large");
  const int c_out = (int)weight.size(0), c_in = (int)weight.size(1), k = (int)weight.size(2);
  const size_t bytes = grpg_conv2d_packed_bytes(c_out, c_in, k);
  TORCH_CHECK(bytes > 0, "detector_pack_weights: k must be 1 or 3 (got ", k, ")");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(weight.device());
  torch::Tensor packed = torch::empty({(int64_t)(bytes / sizeof(float))}, weight.options());
  run("grpg_conv2d_pack_weights", [&](void* stream) {
    return grpg_conv2d_pack_weights(weight.data_ptr<float>(), bias.data_ptr<float>(), c_out, c_in, k,
                                    packed.data_ptr<float>(), stream);
  });
  return packed;
}

// records: a HOST int64 [n, 26] table, one grpg_detector_layer per row in the struct's field order with the pointers as
// integers (detector.py builds it once per plan); arena: any tensor on the plan's device.  One crossing per frame.
void DetectorRun(const torch::Tensor& records, const torch::Tensor& arena) {
  TORCH_CHECK(records.scalar_type() == torch::kInt64 && records.dim() == 2 && records.size(1) == 26 &&
                  records.size(0) >= 1 && records.is_contiguous() && !records.is_cuda(),
              "detector_run: records must be a contiguous host int64 [n, 26] table");
  TORCH_CHECK(arena.is_cuda(), "detector_run: the network's tensors must live on a ROCm/HIP device (torch device "
                               "'cuda'); this op has no CPU path");
  const int64_t n = records.size(0);
  TORCH_CHECK(n < (int64_t(1) << 20), "detector_run: too many layers");
  std::vector<grpg_detector_layer> layers((size_t)n);
  const int64_t* r = records.data_ptr<int64_t>();
  for (int64_t i = 0; i < n; i++, r += 26) {
    for (int j = 0; j < 26; j++)
      if (j != 1 && j != 4 && j != 7 && j != 10 && j != 13)
        TORCH_CHECK(r[j] >= INT32_MIN && r[j] <= INT32_MAX, "detector_run: layer ", i, ": field ", j, " out of range");
    grpg_detector_layer& L = layers[(size_t)i];
    L.kind = (int)r[0];
    L.in = reinterpret_cast<const float*>((uintptr_t)r[1]); L.in_c0 = (int)r[2]; L.in_ct = (int)r[3];
    L.out = reinterpret_cast<float*>((uintptr_t)r[4]); L.out_c0 = (int)r[5]; L.out_ct = (int)r[6];
    L.res = reinterpret_cast<const float*>((uintptr_t)r[7]); L.res_c0 = (int)r[8]; L.res_ct = (int)r[9];
    L.up = reinterpret_cast<float*>((uintptr_t)r[10]); L.up_c0 = (int)r[11]; L.up_ct = (int)r[12];
    L.packed = reinterpret_cast<const float*>((uintptr_t)r[13]);
    L.bs = (int)r[14]; L.c_in = (int)r[15]; L.c_out = (int)r[16];
    L.h_in = (int)r[17]; L.w_in = (int)r[18]; L.h_out = (int)r[19]; L.w_out = (int)r[20];
    L.k = (int)r[21]; L.stride = (int)r[22]; L.act = (int)r[23]; L.in_mode = (int)r[24]; L.tile = (int)r[25];
  }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(arena.device());
  run("grpg_detector_run", [&](void* stream) { return grpg_detector_run(layers.data(), (int)n, stream); });
}

// ---- the detector's network in fp16 (gaussianrpg_amd/detector.py; csrc/detector_f16.hip) ----

// The same float32 weight and bias -> the fp16 network's packed buffer (uint8: a float32 bias block, then fp16).
torch::Tensor DetectorPackWeightsF16(const torch::Tensor& weight, const torch::Tensor& bias) {
  TORCH_CHECK(weight.scalar_type() == torch::kFloat32 && bias.scalar_type() == torch::kFloat32,
              "detector_pack_weights_f16: weight and bias must be float32 (the kernel rounds the weight once)");
  TORCH_CHECK(weight.dim() == 4 && weight.size(2) == weight.size(3) && bias.dim() == 1 && bias.size(0) == weight.size(0) &&
                  weight.is_contiguous() && bias.is_contiguous(),
              "detector_pack_weights_f16: weight must be a contiguous [c_out, c_in, k, k] and bias [c_out] (got ",
              weight.sizes(), " and ", bias.sizes(), ")");
  TORCH_CHECK(weight.is_cuda() && bias.device() == weight.device(),
              "detector_pack_weights_f16: weight and bias must live on one ROCm/HIP device (torch device 'cuda'); this "
              "op has no CPU path");
  TORCH_CHECK(weight.size(0) < (int64_t(1) << 24) && weight.size(1) < (int64_t(1) << 20), "detector_pack_weights_f16: too large");
  const int c_out = (int)weight.size(0), c_in = (int)weight.size(1), k = (int)weight.size(2);
  const size_t bytes = grpg_conv2d_packed_bytes_f16(c_out, c_in, k);
  TORCH_CHECK(bytes > 0, "detector_pack_weights_f16: k must be 1 or 3 (got ", k, ")");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(weight.device());
  torch::Tensor packed = torch::empty({(int64_t)bytes}, weight.options().dtype(torch::kUInt8));
  run("grpg_conv2d_pack_weights_f16", [&](void* stream) {
    return grpg_conv2d_pack_weights_f16(weight.data_ptr<float>(), bias.data_ptr<float>(), c_out, c_in, k,
                                        packed.data_ptr(), stream);
  });
  return packed;
}

// records: a HOST int64 [n, 27] table, one grpg_detector_layer_f16 per row in the struct's field order.
void DetectorRunF16(const torch::Tensor& records, const torch::Tensor& arena) {
  TORCH_CHECK(records.scalar_type() == torch::kInt64 && records.dim() == 2 && records.size(1) == 27 &&
                  records.size(0) >= 1 && records.is_contiguous() && !records.is_cuda(),
              "detector_run_f16: records must be a contiguous host int64 [n, 27] table");
  TORCH_CHECK(arena.is_cuda(), "detector_run_f16: the network's tensors must live on a ROCm/HIP device (torch device "
                               "'cuda'); this op has no CPU path");
  const int64_t n = records.size(0);
  TORCH_CHECK(n < (int64_t(1) << 20), "detector_run_f16: too many layers");
  std::vector<grpg_detector_layer_f16> layers((size_t)n);
  const int64_t* r = records.data_ptr<int64_t>();
  for (int64_t i = 0; i < n; i++, r += 27) {
    for (int j = 0; j < 27; j++)
      if (j != 1 && j != 4 && j != 7 && j != 10 && j != 13)
        TORCH_CHECK(r[j] >= INT32_MIN && r[j] <= INT32_MAX, "detector_run_f16: layer ", i, ": field ", j, " out of range");
    grpg_detector_layer_f16& L = layers[(size_t)i];
    L.kind = (int)r[0];
    L.in = reinterpret_cast<const void*>((uintptr_t)r[1]); L.in_c0 = (int)r[2]; L.in_ct = (int)r[3];
    L.out = reinterpret_cast<void*>((uintptr_t)r[4]); L.out_c0 = (int)r[5]; L.out_ct = (int)r[6];
    L.res = reinterpret_cast<const void*>((uintptr_t)r[7]); L.res_c0 = (int)r[8]; L.res_ct = (int)r[9];
    L.up = reinterpret_cast<void*>((uintptr_t)r[10]); L.up_c0 = (int)r[11]; L.up_ct = (int)r[12];
    L.packed = reinterpret_cast<const void*>((uintptr_t)r[13]);
    L.bs = (int)r[14]; L.c_in = (int)r[15]; L.c_out = (int)r[16];
    L.h_in = (int)r[17]; L.w_in = (int)r[18]; L.h_out = (int)r[19]; L.w_out = (int)r[20];
    L.k = (int)r[21]; L.stride = (int)r[22]; L.act = (int)r[23]; L.in_mode = (int)r[24]; L.tile = (int)r[25];
    L.out_f32 = (int)r[26];
  }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(arena.device());
  run("grpg_detector_run_f16", [&](void* stream) { return grpg_detector_run_f16(layers.data(), (int)n, stream); });
}

// ---- LPIPS (gaussianrpg_amd/lpips.py; csrc/lpips.hip) ----

namespace {
const float* lpips_f32(const torch::Tensor& t, const torch::Device& dev, const char* fn, const char* what) {
  TORCH_CHECK(t.defined(), fn, ": undefined ", what);
  TORCH_CHECK(t.is_cuda(), fn, ": ", what, " must live on a ROCm/HIP device (torch device 'cuda'); this op has no CPU path");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, fn, ": ", what, " must be float32 (got ", t.scalar_type(), "): no hidden cast");
  TORCH_CHECK(t.device() == dev, fn, ": ", what, " is on another device");
  TORCH_CHECK(t.is_contiguous(), fn, ": ", what, " must be contiguous");
  return t.data_ptr<float>();
}
}  // namespace

// float32 [c_out, c_in, k, k] weight and [c_out] bias on the device -> the packed buffer the convolution streams.
torch::Tensor LpipsPackWeights(const torch::Tensor& weight, const torch::Tensor& bias) {
  TORCH_CHECK(weight.defined() && weight.is_cuda(), "lpips_pack_weights: weight must live on a ROCm/HIP device (torch "
              "device 'cuda'); this op has no CPU path");
  const float* w = lpips_f32(weight, weight.device(), "lpips_pack_weights", "weight");
  const float* b = lpips_f32(bias, weight.device(), "lpips_pack_weights", "bias");
  TORCH_CHECK(weight.dim() == 4 && weight.size(2) == weight.size(3) && bias.dim() == 1 && bias.size(0) == weight.size(0),
              "lpips_pack_weights: weight must be [c_out, c_in, k, k] and bias [c_out] (got ", weight.sizes(), " and ",
              bias.sizes(), ")");
  TORCH_CHECK(weight.size(0) < (int64_t(1) << 24) && weight.size(1) < (int64_t(1) << 20), "lpips_pack_weights: too large");
  const int c_out = (int)weight.size(0), c_in = (int)weight.size(1), k = (int)weight.size(2);
  const size_t bytes = grpg_lpips_conv_packed_bytes(c_out, c_in, k);
  TORCH_CHECK(bytes > 0, "lpips_pack_weights: k must be 3, 5 or 11 (got ", k, ")");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(weight.device());
  torch::Tensor packed = torch::empty({(int64_t)(bytes / sizeof(float))}, weight.options());
  run("grpg_lpips_conv_pack_weights", [&](void* stream) {
    return grpg_lpips_conv_pack_weights(w, b, c_out, c_in, k, packed.data_ptr<float>(), stream);
  });
  return packed;
}

int64_t LpipsWorkspaceBytes(const int64_t net, const int64_t pairs, const int64_t h, const int64_t w) {
  if (pairs > INT32_MAX || h > INT32_MAX || w > INT32_MAX || pairs < 0 || h < 0 || w < 0) return 0;
  return (int64_t)grpg_lpips_workspace_bytes((int)net, (int)pairs, (int)h, (int)w);
}

int64_t LpipsWorkspaceMapOffset(const int64_t net, const int64_t pairs, const int64_t h, const int64_t w, const int64_t tap) {
  if (pairs > INT32_MAX || h > INT32_MAX || w > INT32_MAX || pairs < 0 || h < 0 || w < 0) return 0;
  return (int64_t)grpg_lpips_workspace_map_offset((int)net, (int)pairs, (int)h, (int)w, (int)tap);
}

int64_t LpipsTrainWorkspaceBytes(const int64_t net, const int64_t pairs, const int64_t h, const int64_t w) {
  if (pairs > INT32_MAX || h > INT32_MAX || w > INT32_MAX || pairs < 0 || h < 0 || w < 0) return 0;
  return (int64_t)grpg_lpips_train_workspace_bytes((int)net, (int)pairs, (int)h, (int)w);
}

int64_t LpipsTrainActivationOffset(const int64_t net, const int64_t pairs, const int64_t h, const int64_t w, const int64_t conv) {
  if (pairs > INT32_MAX || h > INT32_MAX || w > INT32_MAX || pairs < 0 || h < 0 || w < 0 || conv < 0 || conv > 64) return 0;
  return (int64_t)grpg_lpips_train_activation_offset((int)net, (int)pairs, (int)h, (int)w, (int)conv);
}

// x, y: contiguous float32 [pairs, 3, h, w]; workspace: uint8 of lpips_workspace_bytes; out_pairs [pairs] and out_taps
// [pairs, 5] are the caller's (lpips.py keeps them per shape: no allocation after a shape's first call).
namespace {
void lpips_forward_call(const bool train, const int64_t net, const std::vector<torch::Tensor>& packed,
                        const std::vector<torch::Tensor>& lin, const torch::Tensor& x, const torch::Tensor& y,
                        const torch::Tensor& workspace, const torch::Tensor& out_pairs, const torch::Tensor& out_taps) {
  static const int widths[2][5] = {{64, 192, 384, 256, 256}, {64, 128, 256, 512, 512}};
  TORCH_CHECK(net == GRPG_LPIPS_ALEX || net == GRPG_LPIPS_VGG16, "lpips_forward: unknown net");
  TORCH_CHECK(x.defined() && x.is_cuda(), "lpips_forward: x must live on a ROCm/HIP device (torch device 'cuda'); this op "
              "has no CPU path");
  const torch::Device dev = x.device();
  const float* px = lpips_f32(x, dev, "lpips_forward", "x");
  const float* py = lpips_f32(y, dev, "lpips_forward", "y");
  TORCH_CHECK(x.dim() == 4 && x.size(1) == 3 && x.sizes() == y.sizes(), "lpips_forward: x and y must be [pairs, 3, h, w] of "
              "one shape (got ", x.sizes(), " and ", y.sizes(), ")");
  const int64_t pairs = x.size(0), h = x.size(2), w = x.size(3);
  const int64_t bytes = train ? LpipsTrainWorkspaceBytes(net, pairs, h, w) : LpipsWorkspaceBytes(net, pairs, h, w);
  TORCH_CHECK(bytes > 0, "lpips_forward: ", pairs, " pairs of ", h, " x ", w, " are refused: the image must be at least ",
              net == GRPG_LPIPS_ALEX ? "31 x 31" : "16 x 16", ", pairs in 1 .. 65535 and every layer below 2^31 pixels");
  TORCH_CHECK(packed.size() == (net == GRPG_LPIPS_ALEX ? 5u : 13u) && lin.size() == 5, "lpips_forward: the net takes ",
              net == GRPG_LPIPS_ALEX ? 5 : 13, " packed convolutions and 5 lin weights");
  std::vector<const float*> pp, pl;
  for (const torch::Tensor& t : packed) pp.push_back(lpips_f32(t, dev, "lpips_forward", "packed weights"));
  for (size_t l = 0; l < 5; l++) {
    pl.push_back(lpips_f32(lin[l], dev, "lpips_forward", "lin weights"));
    TORCH_CHECK(lin[l].numel() == widths[net][l], "lpips_forward: lin weights of tap ", l, " have ", lin[l].numel(),
                " elements, the tap has ", widths[net][l], " channels");
  }
  TORCH_CHECK(workspace.defined() && workspace.is_cuda() && workspace.device() == dev && workspace.is_contiguous() &&
                  workspace.scalar_type() == torch::kByte && workspace.numel() >= bytes,
              "lpips_forward: workspace must be a contiguous uint8 tensor of lpips_workspace_bytes (training: "
              "lpips_train_workspace_bytes) on x's device");
  float* po = const_cast<float*>(lpips_f32(out_pairs, dev, "lpips_forward", "out_pairs"));
  float* pt = const_cast<float*>(lpips_f32(out_taps, dev, "lpips_forward", "out_taps"));
  TORCH_CHECK(out_pairs.numel() == pairs && out_taps.numel() == 5 * pairs, "lpips_forward: out_pairs must be [pairs] and "
              "out_taps [pairs, 5]");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  run(train ? "grpg_lpips_forward_train" : "grpg_lpips_forward", [&](void* stream) {
    return (train ? grpg_lpips_forward_train : grpg_lpips_forward)((int)net, pp.data(), pl.data(), px, py, (int)pairs, (int)h,
                                                                    (int)w, workspace.data_ptr(), po, pt, stream);
  });
}
}  // namespace

void LpipsForward(const int64_t net, const std::vector<torch::Tensor>& packed, const std::vector<torch::Tensor>& lin,
                  const torch::Tensor& x, const torch::Tensor& y, const torch::Tensor& workspace,
                  const torch::Tensor& out_pairs, const torch::Tensor& out_taps) {
  lpips_forward_call(false, net, packed, lin, x, y, workspace, out_pairs, out_taps);
}

// The training forward: the same kernels and bits, every convolution's output kept in a workspace of
// lpips_train_workspace_bytes for LpipsBackward.
void LpipsForwardTrain(const int64_t net, const std::vector<torch::Tensor>& packed, const std::vector<torch::Tensor>& lin,
                       const torch::Tensor& x, const torch::Tensor& y, const torch::Tensor& workspace,
                       const torch::Tensor& out_pairs, const torch::Tensor& out_taps) {
  lpips_forward_call(true, net, packed, lin, x, y, workspace, out_pairs, out_taps);
}

// The leaves (tests, tools): ONE convolution + ReLU; zscore: empty, or mean and std (3 + 3 values).
torch::Tensor LpipsConv2d(const torch::Tensor& x, const torch::Tensor& packed, const int64_t c_out, const int64_t k,
                          const int64_t stride, const int64_t pad, const std::vector<double>& zscore, const int64_t tile) {
  TORCH_CHECK(x.defined() && x.is_cuda(), "lpips_conv2d: x must live on a ROCm/HIP device (torch device 'cuda'); this op "
              "has no CPU path");
  const float* px = lpips_f32(x, x.device(), "lpips_conv2d", "x");
  const float* pw = lpips_f32(packed, x.device(), "lpips_conv2d", "packed");
  TORCH_CHECK(x.dim() == 4 && x.numel() > 0, "lpips_conv2d: x must be a non-empty [bs, c_in, h, w]");
  TORCH_CHECK(zscore.empty() || zscore.size() == 6, "lpips_conv2d: zscore is empty or mean[3] + std[3]");
  TORCH_CHECK(x.size(0) <= INT32_MAX && x.size(1) <= INT32_MAX && x.size(2) <= INT32_MAX && x.size(3) <= INT32_MAX &&
                  c_out >= 1 && c_out <= (1 << 24) && stride >= 1 && stride <= 4 && pad >= 0 && pad < k,
              "lpips_conv2d: sizes out of range");
  const int bs = (int)x.size(0), c_in = (int)x.size(1), h = (int)x.size(2), w = (int)x.size(3);
  const size_t bytes = grpg_lpips_conv_packed_bytes((int)c_out, c_in, (int)k);
  TORCH_CHECK(bytes > 0 && (size_t)packed.numel() * sizeof(float) == bytes, "lpips_conv2d: packed does not match c_out, "
              "c_in and k (k must be 3, 5 or 11)");
  TORCH_CHECK(h + 2 * pad >= k && w + 2 * pad >= k, "lpips_conv2d: the input is smaller than the window");
  float mean[3], sdev[3];
  for (size_t i = 0; i < zscore.size() / 2; i++) { mean[i] = (float)zscore[i]; sdev[i] = (float)zscore[3 + i]; }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  torch::Tensor out = torch::empty({bs, c_out, (h + 2 * pad - k) / stride + 1, (w + 2 * pad - k) / stride + 1}, x.options());
  run("grpg_lpips_conv2d", [&](void* stream) {
    return grpg_lpips_conv2d(px, pw, out.data_ptr<float>(), bs, c_in, (int)c_out, h, w, (int)k, (int)stride, (int)pad,
                             zscore.empty() ? nullptr : mean, zscore.empty() ? nullptr : sdev, (int)tile, stream);
  });
  return out;
}

// MaxPool2d(k, 2), k in {2, 3}, no padding, floor mode, of [..., h, w].
torch::Tensor LpipsMaxPool(const torch::Tensor& x, const int64_t k) {
  TORCH_CHECK(x.defined() && x.is_cuda(), "lpips_max_pool: x must live on a ROCm/HIP device (torch device 'cuda'); this "
              "op has no CPU path");
  const float* px = lpips_f32(x, x.device(), "lpips_max_pool", "x");
  TORCH_CHECK(x.dim() == 4 && x.numel() > 0 && (k == 2 || k == 3) && x.size(2) >= k && x.size(3) >= k &&
                  x.size(2) <= INT32_MAX && x.size(3) <= INT32_MAX,
              "lpips_max_pool: x must be [bs, c, h, w] with h, w >= k, and k 2 or 3");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  torch::Tensor out = torch::empty({x.size(0), x.size(1), (x.size(2) - k) / 2 + 1, (x.size(3) - k) / 2 + 1}, x.options());
  run("grpg_lpips_max_pool", [&](void* stream) {
    return grpg_lpips_max_pool(px, out.data_ptr<float>(), (long long)(x.size(0) * x.size(1)), (int)x.size(2), (int)x.size(3),
                               (int)k, stream);
  });
  return out;
}

// One tap: feat [2 * pairs, c, h, w] (x's first), lin [c] -> (mean of s per pair [pairs], s [pairs, h, w]).
std::tuple<torch::Tensor, torch::Tensor> LpipsDistance(const torch::Tensor& feat, const torch::Tensor& lin) {
  TORCH_CHECK(feat.defined() && feat.is_cuda(), "lpips_distance: feat must live on a ROCm/HIP device (torch device "
              "'cuda'); this op has no CPU path");
  const float* pf = lpips_f32(feat, feat.device(), "lpips_distance", "feat");
  const float* pl = lpips_f32(lin, feat.device(), "lpips_distance", "lin");
  TORCH_CHECK(feat.dim() == 4 && feat.numel() > 0 && feat.size(0) % 2 == 0 && lin.numel() == feat.size(1),
              "lpips_distance: feat must be [2 * pairs, c, h, w] and lin hold c weights (got ", feat.sizes(), " and ",
              lin.numel(), ")");
  const int64_t pairs = feat.size(0) / 2, c = feat.size(1), hw = feat.size(2) * feat.size(3);
  TORCH_CHECK(pairs <= 65535 && c <= INT32_MAX && hw < (int64_t(1) << 31) - 256, "lpips_distance: too large");
  const size_t bytes = grpg_lpips_distance_workspace_bytes((int)pairs, (int)c, (int)hw);
  TORCH_CHECK(bytes > 0, "lpips_distance: sizes out of range (at most 768 channels)");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(feat.device());
  torch::Tensor ws = torch::empty({(int64_t)bytes}, feat.options().dtype(torch::kByte));
  torch::Tensor map = torch::empty({pairs, feat.size(2), feat.size(3)}, feat.options());
  torch::Tensor out = torch::empty({pairs}, feat.options());
  run("grpg_lpips_distance", [&](void* stream) {
    return grpg_lpips_distance(pf, pl, (int)pairs, (int)c, (int)hw, ws.data_ptr(), map.data_ptr<float>(),
                               out.data_ptr<float>(), stream);
  });
  return std::make_tuple(out, map);
}

// ---- LPIPS backward (gaussianrpg_amd/lpips.py; csrc/lpips_bwd.hip) ----

namespace {
const float* lpips_opt_f32(const c10::optional<torch::Tensor>& t, const torch::Tensor& like, const char* fn, const char* what) {
  if (!t.has_value() || !t->defined()) return nullptr;
  const float* p = lpips_f32(*t, like.device(), fn, what);
  TORCH_CHECK(t->sizes() == like.sizes(), fn, ": ", what, " must have the produced gradient's shape ", like.sizes(), " (got ",
              t->sizes(), ")");
  return p;
}
}  // namespace

// float32 [c_out, c_in, k, k] on the device -> the layout the backward-data kernel streams (once per model).
torch::Tensor LpipsBwdPackWeights(const torch::Tensor& weight, const int64_t stride) {
  TORCH_CHECK(weight.defined() && weight.is_cuda(), "lpips_bwd_pack_weights: weight must live on a ROCm/HIP device (torch "
              "device 'cuda'); this op has no CPU path");
  const float* w = lpips_f32(weight, weight.device(), "lpips_bwd_pack_weights", "weight");
  TORCH_CHECK(weight.dim() == 4 && weight.size(2) == weight.size(3), "lpips_bwd_pack_weights: weight must be [c_out, c_in, k, k] "
              "(got ", weight.sizes(), ")");
  TORCH_CHECK(weight.size(0) < (int64_t(1) << 20) && weight.size(1) < (int64_t(1) << 20) && stride >= 1 && stride <= 4,
              "lpips_bwd_pack_weights: sizes out of range");
  const int c_out = (int)weight.size(0), c_in = (int)weight.size(1), k = (int)weight.size(2);
  const size_t bytes = grpg_lpips_conv_bwd_packed_bytes(c_out, c_in, k, (int)stride);
  TORCH_CHECK(bytes > 0, "lpips_bwd_pack_weights: the backward covers k 3 or 5 at stride 1, and k 11 at stride 4 with at most "
              "4 input channels (got k ", k, ", stride ", stride, ", c_in ", c_in, ")");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(weight.device());
  torch::Tensor packed = torch::empty({(int64_t)(bytes / sizeof(float))}, weight.options());
  run("grpg_lpips_conv_bwd_pack_weights", [&](void* stream) {
    return grpg_lpips_conv_bwd_pack_weights(w, c_out, c_in, k, (int)stride, packed.data_ptr<float>(), stream);
  });
  return packed;
}

// workspace: the one LpipsForwardTrain filled for this shape; grad_pairs [pairs]; grad_x [pairs, 3, h, w] is the caller's.
void LpipsBackward(const int64_t net, const std::vector<torch::Tensor>& packed_bwd, const std::vector<torch::Tensor>& lin,
                   const torch::Tensor& workspace, const torch::Tensor& grad_pairs, const torch::Tensor& grad_x) {
  TORCH_CHECK(net == GRPG_LPIPS_ALEX || net == GRPG_LPIPS_VGG16, "lpips_backward: unknown net");
  TORCH_CHECK(grad_x.defined() && grad_x.is_cuda(), "lpips_backward: grad_x must live on a ROCm/HIP device (torch device "
              "'cuda'); this op has no CPU path");
  const torch::Device dev = grad_x.device();
  float* pgx = const_cast<float*>(lpips_f32(grad_x, dev, "lpips_backward", "grad_x"));
  const float* pgp = lpips_f32(grad_pairs, dev, "lpips_backward", "grad_pairs");
  TORCH_CHECK(grad_x.dim() == 4 && grad_x.size(1) == 3 && grad_pairs.numel() == grad_x.size(0),
              "lpips_backward: grad_x must be [pairs, 3, h, w] and grad_pairs [pairs] (got ", grad_x.sizes(), " and ",
              grad_pairs.sizes(), ")");
  const int64_t pairs = grad_x.size(0), h = grad_x.size(2), w = grad_x.size(3);
  const int64_t bytes = LpipsTrainWorkspaceBytes(net, pairs, h, w);
  TORCH_CHECK(bytes > 0, "lpips_backward: ", pairs, " pairs of ", h, " x ", w, " are refused: the image must be at least ",
              net == GRPG_LPIPS_ALEX ? "31 x 31" : "16 x 16", ", pairs in 1 .. 65535 and every layer below 2^31 pixels");
  TORCH_CHECK(packed_bwd.size() == (net == GRPG_LPIPS_ALEX ? 5u : 13u) && lin.size() == 5, "lpips_backward: the net takes ",
              net == GRPG_LPIPS_ALEX ? 5 : 13, " packed convolutions and 5 lin weights");
  std::vector<const float*> pp, pl;
  for (const torch::Tensor& t : packed_bwd) pp.push_back(lpips_f32(t, dev, "lpips_backward", "packed weights"));
  for (const torch::Tensor& t : lin) pl.push_back(lpips_f32(t, dev, "lpips_backward", "lin weights"));
  TORCH_CHECK(workspace.defined() && workspace.is_cuda() && workspace.device() == dev && workspace.is_contiguous() &&
                  workspace.scalar_type() == torch::kByte && workspace.numel() >= bytes,
              "lpips_backward: workspace must be the contiguous uint8 tensor of lpips_train_workspace_bytes that "
              "lpips_forward_train filled, on grad_x's device");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  run("grpg_lpips_backward", [&](void* stream) {
    return grpg_lpips_backward((int)net, pp.data(), pl.data(), workspace.data_ptr(), pgp, pgx, (int)pairs, (int)h, (int)w,
                               stream);
  });
}

// The leaves (tests, tools).  ONE convolution backward-data: grad_out [bs, c_out, h_out, w_out] -> [bs, c_in, h_in, w_in];
// act / tap: the ReLU output the gradient lands on and its tap gradient, or None; std: empty, or the z-score's 3 values.
torch::Tensor LpipsConv2dBackwardData(const torch::Tensor& grad_out, const torch::Tensor& packed_bwd,
                                      const c10::optional<torch::Tensor>& act, const c10::optional<torch::Tensor>& tap,
                                      const int64_t c_in, const int64_t h_in, const int64_t w_in, const int64_t k,
                                      const int64_t stride, const int64_t pad, const std::vector<double>& sdev,
                                      const int64_t tile) {
  TORCH_CHECK(grad_out.defined() && grad_out.is_cuda(), "lpips_conv2d_backward_data: grad_out must live on a ROCm/HIP device "
              "(torch device 'cuda'); this op has no CPU path");
  const float* pg = lpips_f32(grad_out, grad_out.device(), "lpips_conv2d_backward_data", "grad_out");
  const float* pw = lpips_f32(packed_bwd, grad_out.device(), "lpips_conv2d_backward_data", "packed_bwd");
  TORCH_CHECK(grad_out.dim() == 4 && grad_out.numel() > 0, "lpips_conv2d_backward_data: grad_out must be a non-empty [bs, c_out, h, w]");
  TORCH_CHECK(sdev.empty() || sdev.size() == 3, "lpips_conv2d_backward_data: std is empty or 3 values");
  TORCH_CHECK(grad_out.size(0) <= 65535 && grad_out.size(1) < (1 << 20) && c_in >= 1 && c_in < (1 << 20) && h_in >= 1 &&
                  w_in >= 1 && h_in <= (1 << 24) && w_in <= (1 << 24) && k >= 1 && k <= 11 && stride >= 1 && stride <= 4 &&
                  pad >= 0 && pad < k,
              "lpips_conv2d_backward_data: sizes out of range");
  const int bs = (int)grad_out.size(0), c_out = (int)grad_out.size(1);
  const size_t bytes = grpg_lpips_conv_bwd_packed_bytes(c_out, (int)c_in, (int)k, (int)stride);
  TORCH_CHECK(bytes > 0 && (size_t)packed_bwd.numel() * sizeof(float) == bytes, "lpips_conv2d_backward_data: packed_bwd does "
              "not match c_out, c_in, k and stride (k 3 or 5 at stride 1, k 11 at stride 4)");
  TORCH_CHECK(h_in + 2 * pad >= k && w_in + 2 * pad >= k && grad_out.size(2) == (h_in + 2 * pad - k) / stride + 1 &&
                  grad_out.size(3) == (w_in + 2 * pad - k) / stride + 1,
              "lpips_conv2d_backward_data: grad_out ", grad_out.sizes(), " is not the convolution's output of a ", h_in, " x ",
              w_in, " input");
  float sd[3] = {1.0f, 1.0f, 1.0f};
  for (size_t i = 0; i < sdev.size(); i++) sd[i] = (float)sdev[i];
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(grad_out.device());
  torch::Tensor out = torch::empty({bs, c_in, h_in, w_in}, grad_out.options());
  const float* pa = lpips_opt_f32(act, out, "lpips_conv2d_backward_data", "act");
  const float* pt = lpips_opt_f32(tap, out, "lpips_conv2d_backward_data", "tap");
  run("grpg_lpips_conv2d_backward_data", [&](void* stream) {
    return grpg_lpips_conv2d_backward_data(pg, pw, pa, pt, out.data_ptr<float>(), bs, (int)c_in, c_out, (int)h_in, (int)w_in,
                                           (int)k, (int)stride, (int)pad, sdev.empty() ? nullptr : sd, (int)tile, stream);
  });
  return out;
}

// MaxPool2d(k, 2) backward in gather form: act [bs, c, h, w] is the pool's input, grad_out its output's gradient.
torch::Tensor LpipsMaxPoolBackward(const torch::Tensor& act, const torch::Tensor& grad_out,
                                   const c10::optional<torch::Tensor>& tap, const int64_t k) {
  TORCH_CHECK(act.defined() && act.is_cuda(), "lpips_max_pool_backward: act must live on a ROCm/HIP device (torch device "
              "'cuda'); this op has no CPU path");
  const float* pa = lpips_f32(act, act.device(), "lpips_max_pool_backward", "act");
  const float* pg = lpips_f32(grad_out, act.device(), "lpips_max_pool_backward", "grad_out");
  TORCH_CHECK(act.dim() == 4 && act.numel() > 0 && (k == 2 || k == 3) && act.size(2) >= k && act.size(3) >= k &&
                  act.size(2) <= INT32_MAX && act.size(3) <= INT32_MAX,
              "lpips_max_pool_backward: act must be [bs, c, h, w] with h, w >= k, and k 2 or 3");
  TORCH_CHECK(grad_out.dim() == 4 && grad_out.size(0) == act.size(0) && grad_out.size(1) == act.size(1) &&
                  grad_out.size(2) == (act.size(2) - k) / 2 + 1 && grad_out.size(3) == (act.size(3) - k) / 2 + 1,
              "lpips_max_pool_backward: grad_out ", grad_out.sizes(), " is not the pool's output of ", act.sizes());
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(act.device());
  torch::Tensor out = torch::empty_like(act);
  const float* pt = lpips_opt_f32(tap, out, "lpips_max_pool_backward", "tap");
  run("grpg_lpips_max_pool_backward", [&](void* stream) {
    return grpg_lpips_max_pool_backward(pa, pg, pt, out.data_ptr<float>(), (long long)(act.size(0) * act.size(1)),
                                        (int)act.size(2), (int)act.size(3), (int)k, stream);
  });
  return out;
}

// One tap's gradient: feat [2 * pairs, c, h, w] (x's first), lin [c], grad_pairs [pairs] -> [pairs, c, h, w].
torch::Tensor LpipsDistanceBackward(const torch::Tensor& feat, const torch::Tensor& lin, const torch::Tensor& grad_pairs) {
  TORCH_CHECK(feat.defined() && feat.is_cuda(), "lpips_distance_backward: feat must live on a ROCm/HIP device (torch device "
              "'cuda'); this op has no CPU path");
  const float* pf = lpips_f32(feat, feat.device(), "lpips_distance_backward", "feat");
  const float* pl = lpips_f32(lin, feat.device(), "lpips_distance_backward", "lin");
  const float* pg = lpips_f32(grad_pairs, feat.device(), "lpips_distance_backward", "grad_pairs");
  TORCH_CHECK(feat.dim() == 4 && feat.numel() > 0 && feat.size(0) % 2 == 0 && lin.numel() == feat.size(1) &&
                  grad_pairs.numel() == feat.size(0) / 2,
              "lpips_distance_backward: feat must be [2 * pairs, c, h, w], lin hold c weights and grad_pairs pairs values");
  const int64_t pairs = feat.size(0) / 2, c = feat.size(1), hw = feat.size(2) * feat.size(3);
  TORCH_CHECK(pairs <= 65535 && c <= 768 && hw < (int64_t(1) << 31) - 256, "lpips_distance_backward: sizes out of range (at "
              "most 768 channels)");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(feat.device());
  torch::Tensor out = torch::empty({pairs, c, feat.size(2), feat.size(3)}, feat.options());
  run("grpg_lpips_distance_backward", [&](void* stream) {
    return grpg_lpips_distance_backward(pf, pl, pg, (int)pairs, (int)c, (int)hw, out.data_ptr<float>(), stream);
  });
  return out;
}

// ---- the closed loop's tail (gaussianrpg_amd/closed_loop.py; csrc/ego_loop.hip) ----

namespace {
// det / count / pos / n and the ranging constants of one call, checked before the device is needed.  params: fy,
// cam_height, k_inv 9, p_inv 16.
struct RangingCall {
  grpg_object_positions_request r{};
  torch::Device device;
  RangingCall(const std::string& who, const torch::Tensor& det, const torch::Tensor& count, const int64_t height,
              const int64_t width, const int64_t nc, const uint64_t mask_lo, const uint64_t mask_hi,
              const std::vector<double>& params, const torch::Tensor& pos, const torch::Tensor& n)
      : device(det.device()) {
    TORCH_CHECK(det.scalar_type() == torch::kFloat32 && det.dim() == 3 && det.size(2) == 6 && det.size(0) >= 1 &&
                    det.is_contiguous(),
                who, ": det must be a contiguous float32 [bs,max_det,6] tensor (got ", det.sizes(), ")");
    const int64_t bs = det.size(0), max_det = det.size(1);
    TORCH_CHECK(max_det >= 1 && max_det <= GRPG_EGO_MAX_DET, who, ": max_det must lie in [1, ", GRPG_EGO_MAX_DET,
                "] (got ", max_det, "): one lane of one wave owns a detection row");
    TORCH_CHECK(nc >= 0 && nc <= GRPG_EGO_MAX_CLASSES, who, ": nc must lie in [0, ", GRPG_EGO_MAX_CLASSES, "] (got ", nc,
                ")");
    TORCH_CHECK(bs < (int64_t(1) << 24), who, ": bs must be below 2^24");
    TORCH_CHECK(det.is_cuda(), who, ": det is on ", det.device(), "; it must live on a ROCm/HIP device (torch device "
                "'cuda'): this op has no CPU path");
    TORCH_CHECK(count.scalar_type() == torch::kInt32 && count.dim() == 1 && count.size(0) == bs &&
                    count.is_contiguous() && count.device() == device,
                who, ": count must be a contiguous int32 [", bs, "] tensor on ", device);
    TORCH_CHECK(pos.scalar_type() == torch::kFloat64 && pos.dim() == 3 && pos.size(0) == bs && pos.size(1) == max_det &&
                    pos.size(2) == 2 && pos.is_contiguous() && pos.device() == device,
                who, ": pos must be a contiguous float64 [", bs, ",", max_det, ",2] tensor on ", device);
    TORCH_CHECK(n.scalar_type() == torch::kInt32 && n.dim() == 1 && n.size(0) == bs && n.is_contiguous() &&
                    n.device() == device,
                who, ": n must be a contiguous int32 [", bs, "] tensor on ", device);
    TORCH_CHECK(params.size() == 27, who, ": the ranging constants are fy, cam_height, k_inv (9) and p_inv (16)");
    TORCH_CHECK(height >= 1 && width >= 1 && height < (1 << 24) && width < (1 << 24), who,
                ": the frame's height and width must lie in [1, 2^24)");
    r.det = det.data_ptr<float>();
    r.count = count.data_ptr<int>();
    r.bs = (int)bs;
    r.max_det = (int)max_det;
    r.pos = pos.data_ptr<double>();
    r.n = n.data_ptr<int>();
    grpg_ranging& g = r.ranging;
    g.height = (int)height;
    g.width = (int)width;
    g.nc = (int)nc;
    g.class_mask[0] = mask_lo;
    g.class_mask[1] = mask_hi;
    g.fy = params[0];
    g.cam_height = params[1];
    std::copy(params.begin() + 2, params.begin() + 11, g.k_inv);
    std::copy(params.begin() + 11, params.end(), g.p_inv);
  }
};
}  // namespace

void ObjectPositions(const torch::Tensor& det, const torch::Tensor& count, const int64_t height, const int64_t width,
                     const int64_t nc, const uint64_t mask_lo, const uint64_t mask_hi, const std::vector<double>& params,
                     const torch::Tensor& pos, const torch::Tensor& n) {
  RangingCall c("object_positions", det, count, height, width, nc, mask_lo, mask_hi, params, pos, n);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(c.device);
  run("grpg_object_positions", [&](void* stream) {
    c.r.hip_stream = stream;
    return grpg_object_positions(&c.r);
  });
}

void EgoLoopStep(const torch::Tensor& det, const torch::Tensor& count, const int64_t height, const int64_t width,
                 const int64_t nc, const uint64_t mask_lo, const uint64_t mask_hi, const std::vector<double>& params,
                 const torch::Tensor& pos, const torch::Tensor& n, const int64_t policy, const int64_t substeps,
                 const double brake_distance, const double cipv_lat_range, const double command,
                 const c10::optional<torch::Tensor>& command_device, const double period, const torch::Tensor& tape,
                 const torch::Tensor& cameras, const std::vector<double>& proj_t, const std::vector<double>& ray_k_inv,
                 const torch::Tensor& state, const c10::optional<torch::Tensor>& log, const int64_t log_index,
                 const torch::Tensor& camera) {
  const std::string who = "ego_loop_step";
  RangingCall c(who, det, count, height, width, nc, mask_lo, mask_hi, params, pos, n);
  const torch::Device device = c.device;
  TORCH_CHECK(policy == GRPG_POLICY_NONE || policy == GRPG_POLICY_AEB, who, ": unknown policy ", policy);
  TORCH_CHECK(substeps >= 1 && substeps < (1 << 20), who, ": substeps must be at least 1 (got ", substeps, ")");
  TORCH_CHECK(period > 0.0 && std::isfinite(period), who, ": period must be positive and finite");
  TORCH_CHECK(tape.scalar_type() == torch::kFloat64 && tape.dim() == 2 && tape.size(0) >= 1 && tape.size(1) == 13 &&
                  tape.is_contiguous() && tape.device() == device && tape.size(0) < (int64_t(1) << 24),
              who, ": tape must be a contiguous float64 [T,13] tensor on ", device);
  const int64_t T = tape.size(0);
  TORCH_CHECK(cameras.scalar_type() == torch::kFloat32 && cameras.dim() == 2 && cameras.size(0) == T &&
                  cameras.size(1) == GRPG_CAMERA_ROW && cameras.is_contiguous() && cameras.device() == device,
              who, ": cameras must be a contiguous float32 [", T, ",", GRPG_CAMERA_ROW, "] tensor on ", device);
  TORCH_CHECK(camera.scalar_type() == torch::kFloat32 && camera.dim() == 1 && camera.size(0) == GRPG_CAMERA_ROW &&
                  camera.is_contiguous() && camera.device() == device,
              who, ": camera must be a contiguous float32 [", GRPG_CAMERA_ROW, "] tensor on ", device);
  TORCH_CHECK(state.scalar_type() == torch::kFloat64 && state.dim() == 1 && state.size(0) == GRPG_EGO_STATE &&
                  state.is_contiguous() && state.device() == device,
              who, ": state must be a contiguous float64 [", GRPG_EGO_STATE, "] tensor on ", device);
  TORCH_CHECK(proj_t.size() == 16 && (ray_k_inv.empty() || ray_k_inv.size() == 9), who,
              ": proj_t holds 16 values, ray_k_inv none or 9");
  grpg_ego_loop_request q{};
  if (log.has_value() && log->defined()) {
    TORCH_CHECK(log->scalar_type() == torch::kFloat64 && log->dim() == 2 && log->size(1) == GRPG_EGO_STATE &&
                    log->is_contiguous() && log->device() == device,
                who, ": log must be a contiguous float64 [steps,", GRPG_EGO_STATE, "] tensor on ", device);
    TORCH_CHECK(log_index >= 0 && log_index < log->size(0), who, ": log index ", log_index, " is outside the log's ",
                log->size(0), " rows");
    q.log = log->data_ptr<double>();
    q.log_rows = log->size(0);
    q.log_index = log_index;
  }
  if (command_device.has_value() && command_device->defined()) {
    TORCH_CHECK(policy == GRPG_POLICY_NONE, who, ": a command is given only with policy=None");
    TORCH_CHECK(command_device->scalar_type() == torch::kFloat64 && command_device->numel() == 1 &&
                    command_device->device() == device,
                who, ": a device command must be a one-element float64 tensor on ", device);
    q.command_device = command_device->data_ptr<double>();
  }
  q.policy = (int)policy;
  q.substeps = (int)substeps;
  q.tape_len = (int)T;
  q.has_ray = ray_k_inv.empty() ? 0 : 1;
  q.brake_distance = brake_distance;
  q.cipv_lat_range = cipv_lat_range;
  q.command = command;
  q.period = period;
  q.tape = tape.data_ptr<double>();
  q.cameras = cameras.data_ptr<float>();
  for (int i = 0; i < 16; ++i) q.proj_t[i] = (float)proj_t[i];
  for (size_t i = 0; i < ray_k_inv.size(); ++i) q.ray_k_inv[i] = ray_k_inv[i];
  q.state = state.data_ptr<double>();
  q.camera = camera.data_ptr<float>();
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  run("grpg_ego_loop_step", [&](void* stream) {
    q.detections = c.r;
    q.detections.hip_stream = stream;
    return grpg_ego_loop_step(&q);
  });
}

// ---- tracklets -> actor poses (gaussianrpg_amd/tracks.py; csrc/tracks.hip) ----

namespace {
// The static table as tracks.TrackTable keeps it: (stamps f64 [F], input_trans f32 [F,M,3], input_rots f32 [F,M,4],
// entries i32 [E,2], entry_offsets i32 [A+1], start f64 [A], end f64 [A]) on the device, entry_offsets i32 [A+1] on the
// host; and one call's per-query arguments.  Everything is checked here, before the device is needed.
struct TrackCall {
  grpg_track_table tb;
  int64_t T;
  const float* opt_trans = nullptr;
  const float* opt_rots = nullptr;
  const double* val = nullptr;

  TrackCall(const char* what, const std::vector<torch::Tensor>& table, const torch::Tensor& timestamps,
            const torch::Tensor& ego, const c10::optional<torch::Tensor>& opt_trans_t,
            const c10::optional<torch::Tensor>& opt_rots_t, const c10::optional<torch::Tensor>& val_stamps) {
    TORCH_CHECK(table.size() == 8, what, ": the table is (stamps, input_trans, input_rots, entries, entry_offsets, "
                                         "start, end, entry_offsets on the host)");
    const torch::Tensor &stamps = table[0], &itr = table[1], &irot = table[2], &entries = table[3], &offs = table[4],
                        &start = table[5], &end = table[6], &offs_host = table[7];
    auto is = [](const torch::Tensor& t, const torch::ScalarType ty) { return t.scalar_type() == ty && t.is_contiguous(); };
    TORCH_CHECK(is(stamps, torch::kFloat64) && stamps.dim() == 1 && stamps.size(0) > 0, what,
                ": stamps must be a contiguous float64 [F] tensor (float32 cannot tell neighbouring stamps apart)");
    const int64_t F = stamps.size(0);
    TORCH_CHECK(is(itr, torch::kFloat32) && itr.dim() == 3 && itr.size(0) == F && itr.size(1) > 0 && itr.size(2) == 3,
                what, ": input_trans must be a contiguous float32 [F,M,3] tensor");
    const int64_t M = itr.size(1);
    TORCH_CHECK(is(irot, torch::kFloat32) && irot.dim() == 3 && irot.size(0) == F && irot.size(1) == M &&
                    irot.size(2) == 4, what, ": input_rots must be a contiguous float32 [F,M,4] tensor");
    TORCH_CHECK(is(entries, torch::kInt32) && entries.dim() == 2 && entries.size(1) == 2, what,
                ": entries must be a contiguous int32 [E,2] tensor");
    TORCH_CHECK(is(offs, torch::kInt32) && offs.dim() == 1 && offs.size(0) >= 2, what,
                ": entry_offsets must be a contiguous int32 [A+1] tensor");
    const int64_t A = offs.size(0) - 1;
    TORCH_CHECK(is(start, torch::kFloat64) && is(end, torch::kFloat64) && start.dim() == 1 && end.dim() == 1 &&
                    start.size(0) == A && end.size(0) == A, what, ": start / end must be contiguous float64 [A] tensors");
    TORCH_CHECK(is(offs_host, torch::kInt32) && offs_host.dim() == 1 && offs_host.size(0) == A + 1 &&
                    offs_host.device().is_cpu(), what, ": the host copy of entry_offsets must be an int32 [A+1] CPU tensor");
    TORCH_CHECK(F * M <= (int64_t(1) << 27) && A <= 65536, what, ": F * M <= 2^27 and A <= 65536");
    TORCH_CHECK(is(timestamps, torch::kFloat64) && timestamps.dim() == 1 && timestamps.size(0) > 0, what,
                ": timestamps must be a contiguous float64 [T] tensor");
    T = timestamps.size(0);
    TORCH_CHECK(T * A <= (int64_t(1) << 24), what, ": T * A <= 2^24");
    TORCH_CHECK(is(ego, torch::kFloat32) && ego.dim() == 3 && ego.size(0) == T && ego.size(1) == 4 && ego.size(2) == 4,
                what, ": ego must be a contiguous float32 [T,4,4] tensor");
    const bool has_t = opt_trans_t.has_value() && opt_trans_t->defined();
    const bool has_r = opt_rots_t.has_value() && opt_rots_t->defined();
    TORCH_CHECK(has_t == has_r, what, ": opt_trans and opt_rots come together or not at all");
    const bool has_v = val_stamps.has_value() && val_stamps->defined();
    TORCH_CHECK(!has_v || has_t, what, ": val_stamps needs opt_trans / opt_rots");
    if (has_t) {
      TORCH_CHECK(is(*opt_trans_t, torch::kFloat32) && opt_trans_t->sizes() == itr.sizes(),
                  what, ": opt_trans must be a contiguous float32 [F,M,3] tensor");
      TORCH_CHECK(is(*opt_rots_t, torch::kFloat32) && opt_rots_t->dim() == 3 && opt_rots_t->size(0) == F &&
                      opt_rots_t->size(1) == M && opt_rots_t->size(2) == 1,
                  what, ": opt_rots must be a contiguous float32 [F,M,1] tensor");
    }
    if (has_v)
      TORCH_CHECK(is(*val_stamps, torch::kFloat64) && val_stamps->dim() == 3 && val_stamps->size(0) == T &&
                      val_stamps->size(1) == A && val_stamps->size(2) == 2,
                  what, ": val_stamps must be a contiguous float64 [T,A,2] tensor");
    TORCH_CHECK(stamps.is_cuda(), what, ": the table must live on a ROCm/HIP device (torch device 'cuda'); this op "
                                        "has no CPU path");
    const torch::Device dev = stamps.device();
    for (const torch::Tensor* t : {&itr, &irot, &entries, &offs, &start, &end, &timestamps, &ego})
      TORCH_CHECK(t->device() == dev, what, ": every device tensor must be on ", dev);
    if (has_t) {
      TORCH_CHECK(opt_trans_t->device() == dev && opt_rots_t->device() == dev, what,
                  ": opt_trans and opt_rots must be on ", dev);
      opt_trans = opt_trans_t->data_ptr<float>();
      opt_rots = opt_rots_t->data_ptr<float>();
    }
    if (has_v) {
      TORCH_CHECK(val_stamps->device() == dev, what, ": val_stamps must be on ", dev);
      val = val_stamps->data_ptr<double>();
    }
    tb.F = (int)F; tb.M = (int)M; tb.A = (int)A; tb.E = (int)entries.size(0);
    tb.stamps = stamps.data_ptr<double>();
    tb.input_trans = itr.data_ptr<float>();
    tb.input_rots = irot.data_ptr<float>();
    tb.entries = entries.data_ptr<int>();
    tb.entry_offsets = offs.data_ptr<int>();
    tb.start = start.data_ptr<double>();
    tb.end = end.data_ptr<double>();
    tb.entry_offsets_host = offs_host.data_ptr<int>();
  }
};
}  // namespace

// -> (rot f32 [T,A,4], trans f32 [T,A,3], active u8 [T,A], chosen i32 [T,A,4]); one launch, no host wait
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> TrackPosesForward(
    const std::vector<torch::Tensor>& table, const torch::Tensor& timestamps, const torch::Tensor& ego,
    const c10::optional<torch::Tensor>& opt_trans, const c10::optional<torch::Tensor>& opt_rots,
    const c10::optional<torch::Tensor>& val_stamps) {
  const char* what = "track_poses_forward";
  const TrackCall c(what, table, timestamps, ego, opt_trans, opt_rots, val_stamps);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(ego.device());
  const int64_t A = c.tb.A;
  torch::Tensor rot = torch::empty({c.T, A, 4}, ego.options());
  torch::Tensor trans = torch::empty({c.T, A, 3}, ego.options());
  torch::Tensor active = torch::empty({c.T, A}, ego.options().dtype(torch::kUInt8));
  torch::Tensor chosen = torch::empty({c.T, A, 4}, ego.options().dtype(torch::kInt32));
  run("grpg_track_poses_forward", [&](void* stream) {
    return grpg_track_poses_forward(&c.tb, (int)c.T, timestamps.data_ptr<double>(), ego.data_ptr<float>(), c.opt_trans,
                                    c.opt_rots, c.val, rot.data_ptr<float>(), trans.data_ptr<float>(),
                                    active.data_ptr<uint8_t>(), chosen.data_ptr<int>(), stream);
  });
  return std::make_tuple(rot, trans, active, chosen);
}

// -> (g_opt_trans f32 [F,M,3], g_opt_rots f32 [F,M,1]): dense, two views of one allocation; one memset, one launch
std::tuple<torch::Tensor, torch::Tensor> TrackPosesBackward(
    const std::vector<torch::Tensor>& table, const torch::Tensor& timestamps, const torch::Tensor& ego,
    const torch::Tensor& opt_trans, const torch::Tensor& opt_rots, const c10::optional<torch::Tensor>& val_stamps,
    const torch::Tensor& g_rot, const torch::Tensor& g_trans) {
  const char* what = "track_poses_backward";
  const TrackCall c(what, table, timestamps, ego, opt_trans, opt_rots, val_stamps);
  const int64_t A = c.tb.A, F = c.tb.F, M = c.tb.M;
  for (const auto& [g, n, name] : {std::make_tuple(&g_rot, int64_t(4), "g_rot"), std::make_tuple(&g_trans, int64_t(3), "g_trans")})
    TORCH_CHECK(g->scalar_type() == torch::kFloat32 && g->is_contiguous() && g->dim() == 3 && g->size(0) == c.T &&
                    g->size(1) == A && g->size(2) == n && g->device() == ego.device(),
                what, ": ", name, " must be a contiguous float32 [T,A,", n, "] tensor on ", ego.device());
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(ego.device());
  torch::Tensor both = torch::empty({F * M * 4}, ego.options());
  torch::Tensor g_ot = both.narrow(0, 0, F * M * 3).view({F, M, 3});
  torch::Tensor g_or = both.narrow(0, F * M * 3, F * M).view({F, M, 1});
  run("grpg_track_poses_backward", [&](void* stream) {
    return grpg_track_poses_backward(&c.tb, (int)c.T, timestamps.data_ptr<double>(), ego.data_ptr<float>(), c.opt_trans,
                                     c.opt_rots, c.val, g_rot.data_ptr<float>(), g_trans.data_ptr<float>(),
                                     g_ot.data_ptr<float>(), g_or.data_ptr<float>(), stream);
  });
  return std::make_tuple(g_ot, g_or);
}

std::tuple<std::vector<float>, int> StageTiming() {
  std::vector<float> ms(GRPG_NUM_STAGES, 0.f);
  int calls = 0;
  const int rc = grpg_get_stage_timing(ms.data(), &calls);
  if (rc != GRPG_OK) raise_abi_error("grpg_get_stage_timing", rc);
  return std::make_tuple(ms, calls);
}

std::tuple<float, float, int> BackwardTiming() {
  float blend = 0.f, pre = 0.f;
  int calls = 0;
  const int rc = grpg_get_backward_timing(&blend, &pre, &calls);
  if (rc != GRPG_OK) raise_abi_error("grpg_get_backward_timing", rc);
  return std::make_tuple(blend, pre, calls);
}

// simple_knn._C.distCUDA2 (submodules/simple-knn/spatial.cu:14-25): [P,3] points -> [P] mean
// squared distance to the 3 nearest other points.
torch::Tensor distCUDA2(const torch::Tensor& points) {
  require_device(points);
  TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "points must be [P,3]");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(points.device());
  const int P = points.size(0);
  auto float_opts = points.options().dtype(torch::kFloat32);
  torch::Tensor pts = points.to(torch::kFloat32).contiguous();
  torch::Tensor means = torch::zeros({P}, float_opts);   // the reference returns torch::full(0)
  torch::Tensor workspace = torch::empty({0}, points.options().dtype(torch::kByte));
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int rc = grpg_knn_mean_dist2(P, pts.data_ptr<float>(), means.data_ptr<float>(), resize_blob,
                                     &workspace, (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_knn_mean_dist2", rc);
  return means;
}

// ---- the pieces every loss binding is made of ----
namespace {
// One loss call of the C ABI, as run(): on the current stream, the GIL released (the C calls touch no Python object).
template <class Call>
void loss_call(const char* what, Call&& call) {
  if (const int rc = run(what, call); rc != GRPG_OK) raise_abi_error(what, rc);
}

torch::Tensor loss_workspace(const size_t bytes, const torch::Device& dev) {
  return torch::empty({(long long)bytes}, torch::TensorOptions().dtype(torch::kByte).device(dev));
}

// The upstream gradient of a stats vector as the kernels read it.  count: the elements it must have (0: at least one).
torch::Tensor loss_grad_stats(const torch::Tensor& grad_stats, const torch::Device& dev, const int64_t count,
                              const char* mismatch) {
  torch::Tensor g = grad_stats.to(dev, torch::kFloat32).contiguous();
  TORCH_CHECK(count ? g.numel() == count : g.numel() >= 1, mismatch);
  return g;
}

// Fused SSIM + L1 loss (gaussianrpg_amd/loss.py).  img1 / img2: float32 [B,C,H,W] on one device (made contiguous
// here); mask: empty or uint8 [1|B, 1|C, H, W].  Returns (stats [4 + B], saved partials [3,B,C,H,W] or empty).
struct SsimIn {
  torch::Tensor a, b, m;   // contiguous
  int B, C, H, W;
  const unsigned char* mask = nullptr;   // NULL: no mask
  int mask_batch = 1, mask_channels = 1;
};

SsimIn ssim_args(const torch::Tensor& img1, const torch::Tensor& img2, const torch::Tensor& mask) {
  TORCH_CHECK(img1.is_cuda() && img2.is_cuda(), "ssim: images must live on a ROCm/HIP device (no CPU path)");
  TORCH_CHECK(img1.scalar_type() == torch::kFloat32 && img2.scalar_type() == torch::kFloat32,
              "ssim: images must be float32");
  TORCH_CHECK(img1.dim() == 4 && img1.sizes() == img2.sizes(), "ssim: images must be two [B,C,H,W] of one shape");
  TORCH_CHECK(img1.device() == img2.device(), "ssim: images on different devices");
  SsimIn in;
  in.a = img1.contiguous();
  in.b = img2.contiguous();
  in.B = in.a.size(0); in.C = in.a.size(1); in.H = in.a.size(2); in.W = in.a.size(3);
  if (mask.defined() && mask.numel() > 0) {
    TORCH_CHECK(mask.device() == img1.device() && mask.scalar_type() == torch::kUInt8 && mask.dim() == 4 &&
                    mask.size(2) == img1.size(2) && mask.size(3) == img1.size(3),
                "ssim: mask must be uint8 [1|B, 1|C, H, W] on the images' device");
    in.m = mask.contiguous();
    in.mask = in.m.data_ptr<uint8_t>();
    in.mask_batch = in.m.size(0);
    in.mask_channels = in.m.size(1);
  }
  return in;
}
}  // namespace

std::tuple<torch::Tensor, torch::Tensor> SsimForward(const torch::Tensor& img1, const torch::Tensor& img2,
                                                     const torch::Tensor& mask, const double w_l1,
                                                     const double w_ssim, const bool save_partials) {
  const SsimIn in = ssim_args(img1, img2, mask);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.a.device());
  auto fopts = in.a.options();
  torch::Tensor stats = torch::empty({4 + in.B}, fopts);
  torch::Tensor saved = save_partials ? torch::empty({3, in.B, in.C, in.H, in.W}, fopts) : torch::empty({0}, fopts);
  const size_t ws_bytes = grpg_ssim_workspace_bytes(in.B, in.C, in.H, in.W);
  torch::Tensor ws = loss_workspace(ws_bytes > 0 ? ws_bytes : 8, in.a.device());
  loss_call("grpg_ssim_forward", [&](void* stream) {
    return grpg_ssim_forward(in.B, in.C, in.H, in.W, in.a.data_ptr<float>(), in.b.data_ptr<float>(), in.mask,
                             in.mask_batch, in.mask_channels, (float)w_l1, (float)w_ssim, stats.data_ptr<float>(),
                             save_partials ? saved.data_ptr<float>() : nullptr, ws.data_ptr(), stream);
  });
  return std::make_tuple(stats, saved);
}

torch::Tensor SsimBackward(const torch::Tensor& img1, const torch::Tensor& img2, const torch::Tensor& mask,
                           const double w_l1, const double w_ssim, const torch::Tensor& stats,
                           const torch::Tensor& saved, const torch::Tensor& grad_stats) {
  const SsimIn in = ssim_args(img1, img2, mask);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.a.device());
  TORCH_CHECK(stats.numel() == 4 + in.B && saved.numel() == 3 * in.a.numel(),
              "ssim_backward: stats / saved do not match");
  const torch::Tensor g = loss_grad_stats(grad_stats, in.a.device(), 4 + in.B,
                                          "ssim_backward: grad_stats must have 4 + B elements");
  torch::Tensor grad = torch::empty_like(in.a);
  loss_call("grpg_ssim_backward", [&](void* stream) {
    return grpg_ssim_backward(in.B, in.C, in.H, in.W, in.a.data_ptr<float>(), in.b.data_ptr<float>(), in.mask,
                              in.mask_batch, in.mask_channels, (float)w_l1, (float)w_ssim, stats.data_ptr<float>(),
                              saved.data_ptr<float>(), g.data_ptr<float>(), grad.data_ptr<float>(), stream);
  });
  return grad;
}

// Fused lidar-depth / sky / object-alpha losses (gaussianrpg_amd/loss.py).  Every plane is empty (absent) or a
// contiguous H*W tensor on one device: float32 for depth / acc / lidar_depth / acc_obj, uint8 for the masks.
// Returns (stats [9], workspace); the workspace carries the selection state to the backward.
namespace {
struct AuxIn {
  int H, W;
  torch::Device dev = torch::kCPU;
};

const float* aux_f(const torch::Tensor& t) { return t.numel() ? t.data_ptr<float>() : nullptr; }
const unsigned char* aux_u8(const torch::Tensor& t) { return t.numel() ? t.data_ptr<uint8_t>() : nullptr; }

AuxIn aux_args(const int64_t H, const int64_t W, const std::vector<torch::Tensor>& planes,
               const std::vector<torch::Tensor>& masks) {
  AuxIn in;
  TORCH_CHECK(H > 0 && W > 0 && H * W <= 0x7FFFFFFFll, "aux_loss: H and W must be positive with H*W < 2^31");
  in.H = (int)H;
  in.W = (int)W;
  bool any = false;
  auto check = [&](const torch::Tensor& t, const c10::ScalarType ty, const char* what) {
    if (!t.defined() || t.numel() == 0) return;
    TORCH_CHECK(t.is_cuda(), "aux_loss: ", what, " must live on a ROCm/HIP device (no CPU path)");
    TORCH_CHECK(t.scalar_type() == ty && t.numel() == H * W && t.is_contiguous(), "aux_loss: ", what,
                " must be a contiguous ", ty == torch::kFloat32 ? "float32" : "uint8", " plane of H*W elements");
    if (any) TORCH_CHECK(t.device() == in.dev, "aux_loss: planes on different devices");
    in.dev = t.device();
    any = true;
  };
  for (const auto& t : planes) check(t, torch::kFloat32, "plane");
  for (const auto& t : masks) check(t, torch::kUInt8, "mask");
  TORCH_CHECK(any, "aux_loss: no input plane");
  return in;
}
}  // namespace

std::tuple<torch::Tensor, torch::Tensor> AuxLossForward(
    const int64_t H, const int64_t W, const torch::Tensor& depth, const torch::Tensor& acc,
    const torch::Tensor& lidar, const torch::Tensor& mask, const torch::Tensor& sky, const torch::Tensor& acc_obj,
    const torch::Tensor& bound, const double sky_scale, const double lam_lidar, const double lam_sky,
    const double lam_reg) {
  const AuxIn in = aux_args(H, W, {depth, acc, lidar, acc_obj}, {mask, sky, bound});
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.dev);
  auto fopts = torch::TensorOptions().dtype(torch::kFloat32).device(in.dev);
  torch::Tensor stats = torch::empty({9}, fopts);
  torch::Tensor ws = loss_workspace(grpg_aux_loss_workspace_bytes(in.H, in.W), in.dev);
  loss_call("grpg_aux_loss_forward", [&](void* stream) {
    return grpg_aux_loss_forward(in.H, in.W, aux_f(depth), aux_f(acc), aux_f(lidar), aux_u8(mask), aux_u8(sky),
                                 aux_f(acc_obj), aux_u8(bound), (float)sky_scale, (float)lam_lidar, (float)lam_sky,
                                 (float)lam_reg, stats.data_ptr<float>(), ws.data_ptr(), stream);
  });
  return std::make_tuple(stats, ws);
}

// Returns (grad_depth, grad_acc, grad_acc_obj), each [H*W] or empty when not wanted.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> AuxLossBackward(
    const int64_t H, const int64_t W, const torch::Tensor& depth, const torch::Tensor& acc,
    const torch::Tensor& lidar, const torch::Tensor& mask, const torch::Tensor& sky, const torch::Tensor& acc_obj,
    const torch::Tensor& bound, const double sky_scale, const double lam_lidar, const double lam_sky,
    const double lam_reg, const torch::Tensor& grad_stats, const torch::Tensor& ws, const bool want_depth,
    const bool want_acc, const bool want_acc_obj) {
  const AuxIn in = aux_args(H, W, {depth, acc, lidar, acc_obj}, {mask, sky, bound});
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.dev);
  TORCH_CHECK(ws.device() == in.dev && (size_t)ws.numel() == grpg_aux_loss_workspace_bytes(in.H, in.W),
              "aux_loss_backward: workspace does not match");
  const torch::Tensor g = loss_grad_stats(grad_stats, in.dev, 9, "aux_loss_backward: grad_stats must have 9 elements");
  auto fopts = torch::TensorOptions().dtype(torch::kFloat32).device(in.dev);
  auto plane = [&](bool want) { return want ? torch::empty({H * W}, fopts) : torch::empty({0}, fopts); };
  torch::Tensor gd = plane(want_depth), ga = plane(want_acc), go = plane(want_acc_obj);
  loss_call("grpg_aux_loss_backward", [&](void* stream) {
    return grpg_aux_loss_backward(in.H, in.W, aux_f(depth), aux_f(acc), aux_f(lidar), aux_u8(mask), aux_u8(sky),
                                  aux_f(acc_obj), aux_u8(bound), (float)sky_scale, (float)lam_lidar, (float)lam_sky,
                                  (float)lam_reg, g.data_ptr<float>(), ws.data_ptr(),
                                  want_depth ? gd.data_ptr<float>() : nullptr,
                                  want_acc ? ga.data_ptr<float>() : nullptr,
                                  want_acc_obj ? go.data_ptr<float>() : nullptr, stream);
  });
  return std::make_tuple(gd, ga, go);
}

// Fused semantic cross-entropy loss (gaussianrpg_amd/loss.py).  semantic: contiguous float32 [S,H,W]; target:
// contiguous int64 or int32 [H,W] on the same device; mode 0 = logits, 1 = probabilities (raw planes).
// Returns (stats [4], workspace, labels uint8 [H,W] or empty); the workspace carries n_valid and the per-pixel
// logsumexp to the backward.
namespace {
struct SemIn {
  int S, H, W, target_bytes;
};

SemIn semantic_args(const char* fn, const torch::Tensor& semantic, const torch::Tensor& target, const int64_t mode) {
  TORCH_CHECK(semantic.defined() && target.defined(), fn, ": undefined tensor");
  TORCH_CHECK(semantic.is_cuda() && target.is_cuda(), fn,
              ": semantic and target must live on a ROCm/HIP device (no CPU path)");
  TORCH_CHECK(semantic.device() == target.device(), fn, ": semantic and target on different devices");
  TORCH_CHECK(semantic.scalar_type() == torch::kFloat32 && semantic.dim() == 3 && semantic.is_contiguous(), fn,
              ": semantic must be a contiguous float32 [S,H,W] tensor");
  TORCH_CHECK((target.scalar_type() == torch::kInt64 || target.scalar_type() == torch::kInt32) &&
                  target.dim() == 2 && target.is_contiguous(),
              fn, ": target must be a contiguous int64 or int32 [H,W] tensor");
  TORCH_CHECK(target.size(0) == semantic.size(1) && target.size(1) == semantic.size(2), fn,
              ": target must have the H x W of semantic");
  TORCH_CHECK(semantic.size(0) >= 1 && semantic.size(0) <= 0x7FFFFFFFll, fn, ": S must be at least 1");
  const int64_t H = semantic.size(1), W = semantic.size(2);
  TORCH_CHECK(H > 0 && W > 0 && H * W <= 0x7FFFFFFFll, fn, ": H and W must be positive with H*W < 2^31");
  TORCH_CHECK(mode == 0 || mode == 1, fn, ": mode must be 0 (logits) or 1 (probabilities)");
  return SemIn{(int)semantic.size(0), (int)H, (int)W, target.scalar_type() == torch::kInt64 ? 8 : 4};
}
}  // namespace

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> SemanticCeForward(
    const torch::Tensor& semantic, const torch::Tensor& target, const int64_t mode, const bool want_labels) {
  const SemIn in = semantic_args("semantic_ce_forward", semantic, target, mode);
  TORCH_CHECK(!want_labels || in.S <= 256, "semantic_ce_forward: the uint8 label plane needs S <= 256");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(semantic.device());
  auto fopts = torch::TensorOptions().dtype(torch::kFloat32).device(semantic.device());
  torch::Tensor stats = torch::empty({4}, fopts);
  torch::Tensor ws = loss_workspace(grpg_semantic_ce_workspace_bytes(in.H, in.W), semantic.device());
  torch::Tensor labels = want_labels ? torch::empty({in.H, in.W}, fopts.dtype(torch::kByte))
                                     : torch::empty({0}, fopts.dtype(torch::kByte));
  loss_call("grpg_semantic_ce_forward", [&](void* stream) {
    return grpg_semantic_ce_forward(in.S, in.H, in.W, semantic.data_ptr<float>(), target.data_ptr(), in.target_bytes,
                                    (int)mode, stats.data_ptr<float>(),
                                    want_labels ? labels.data_ptr<uint8_t>() : nullptr, ws.data_ptr(), stream);
  });
  return std::make_tuple(stats, ws, labels);
}

// grad_stats: the upstream gradient of the stats vector (entry 0, the loss, is used).  grad_out: None, or a
// contiguous float32 tensor of S*H*W elements to write into (every element is overwritten).
torch::Tensor SemanticCeBackward(const torch::Tensor& semantic, const torch::Tensor& target, const int64_t mode,
                                 const torch::Tensor& grad_stats, const torch::Tensor& ws,
                                 const c10::optional<torch::Tensor>& grad_out) {
  const SemIn in = semantic_args("semantic_ce_backward", semantic, target, mode);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(semantic.device());
  TORCH_CHECK(ws.device() == semantic.device() && ws.scalar_type() == torch::kByte && ws.is_contiguous() &&
                  (size_t)ws.numel() == grpg_semantic_ce_workspace_bytes(in.H, in.W),
              "semantic_ce_backward: workspace does not match");
  const torch::Tensor g = loss_grad_stats(grad_stats, semantic.device(), 0, "semantic_ce_backward: grad_stats is empty");
  torch::Tensor grad;
  if (grad_out) {
    grad = *grad_out;
    TORCH_CHECK(grad.device() == semantic.device() && grad.scalar_type() == torch::kFloat32 &&
                    grad.is_contiguous() && grad.numel() == semantic.numel(),
                "semantic_ce_backward: grad_out must be a contiguous float32 tensor of S*H*W elements on the device");
  } else {
    grad = torch::empty_like(semantic);
  }
  loss_call("grpg_semantic_ce_backward", [&](void* stream) {
    return grpg_semantic_ce_backward(in.S, in.H, in.W, semantic.data_ptr<float>(), target.data_ptr(), in.target_bytes,
                                     (int)mode, g.data_ptr<float>(), ws.data_ptr(), grad.data_ptr<float>(), stream);
  });
  return grad;
}

// Fused mono-normal loss (gaussianrpg_amd/loss.py).  normals / mono: contiguous float32 [3,H,W]; wvt: the camera's
// float32 [4,4] (or [3,3]) device tensor, any strides (read on the device); mask / sky: empty or contiguous uint8 of
// H*W elements.  Returns (stats [4], workspace).
namespace {
struct NormalIn {
  int H, W, rs, cs;
  const unsigned char *mask, *sky;
};

NormalIn normal_args(const char* fn, const torch::Tensor& normals, const torch::Tensor& mono, const torch::Tensor& wvt,
                     const torch::Tensor& mask, const torch::Tensor& sky, const int64_t top_rows) {
  TORCH_CHECK(normals.defined() && mono.defined() && wvt.defined(), fn, ": undefined tensor");
  TORCH_CHECK(normals.is_cuda() && mono.is_cuda() && wvt.is_cuda(), fn,
              ": normals, mono_normal and world_view_transform must live on a ROCm/HIP device (no CPU path)");
  TORCH_CHECK(normals.device() == mono.device() && normals.device() == wvt.device(), fn, ": tensors on different devices");
  TORCH_CHECK(normals.scalar_type() == torch::kFloat32 && normals.dim() == 3 && normals.size(0) == 3 &&
                  normals.is_contiguous(), fn, ": normals must be a contiguous float32 [3,H,W] tensor");
  TORCH_CHECK(mono.scalar_type() == torch::kFloat32 && mono.is_contiguous() && mono.sizes() == normals.sizes(), fn,
              ": mono_normal must be a contiguous float32 tensor of the shape of normals");
  TORCH_CHECK(wvt.scalar_type() == torch::kFloat32 && wvt.dim() == 2 && wvt.size(0) >= 3 && wvt.size(1) >= 3, fn,
              ": world_view_transform must be a float32 [4,4] tensor");
  const int64_t H = normals.size(1), W = normals.size(2);
  TORCH_CHECK(H > 0 && W > 0 && H * W <= 0x7FFFFFFFll, fn, ": H and W must be positive with H*W < 2^31");
  TORCH_CHECK(top_rows >= 0 && top_rows <= 0x7FFFFFFFll, fn, ": top_rows must not be negative");
  NormalIn in{(int)H, (int)W, (int)wvt.stride(0), (int)wvt.stride(1), nullptr, nullptr};
  auto plane = [&](const torch::Tensor& m, const char* what) -> const unsigned char* {
    if (!m.defined() || m.numel() == 0) return nullptr;
    TORCH_CHECK(m.is_cuda() && m.device() == normals.device() && m.scalar_type() == torch::kUInt8 &&
                    m.is_contiguous() && m.numel() == H * W,
                fn, ": ", what, " must be a contiguous uint8 plane of H*W elements on the device of normals");
    return m.data_ptr<uint8_t>();
  };
  in.mask = plane(mask, "mask");
  in.sky = plane(sky, "sky_mask");
  return in;
}
}  // namespace

std::tuple<torch::Tensor, torch::Tensor> NormalLossForward(const torch::Tensor& normals, const torch::Tensor& mono,
                                                           const torch::Tensor& wvt, const torch::Tensor& mask,
                                                           const torch::Tensor& sky, const bool normalize,
                                                           const int64_t top_rows) {
  const NormalIn in = normal_args("normal_loss_forward", normals, mono, wvt, mask, sky, top_rows);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(normals.device());
  torch::Tensor stats = torch::empty({4}, torch::TensorOptions().dtype(torch::kFloat32).device(normals.device()));
  torch::Tensor ws = loss_workspace(grpg_normal_loss_workspace_bytes(in.H, in.W), normals.device());
  loss_call("grpg_normal_loss_forward", [&](void* stream) {
    return grpg_normal_loss_forward(in.H, in.W, normals.data_ptr<float>(), mono.data_ptr<float>(),
                                    wvt.data_ptr<float>(), in.rs, in.cs, in.mask, in.sky, normalize ? 1 : 0,
                                    (int)top_rows, stats.data_ptr<float>(), ws.data_ptr(), stream);
  });
  return std::make_tuple(stats, ws);
}

torch::Tensor NormalLossBackward(const torch::Tensor& normals, const torch::Tensor& mono, const torch::Tensor& wvt,
                                 const torch::Tensor& mask, const torch::Tensor& sky, const bool normalize,
                                 const int64_t top_rows, const torch::Tensor& grad_stats, const torch::Tensor& ws) {
  const NormalIn in = normal_args("normal_loss_backward", normals, mono, wvt, mask, sky, top_rows);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(normals.device());
  TORCH_CHECK(ws.device() == normals.device() && ws.scalar_type() == torch::kByte && ws.is_contiguous() &&
                  (size_t)ws.numel() == grpg_normal_loss_workspace_bytes(in.H, in.W),
              "normal_loss_backward: workspace does not match");
  const torch::Tensor g = loss_grad_stats(grad_stats, normals.device(), 4,
                                          "normal_loss_backward: grad_stats must have 4 elements");
  torch::Tensor grad = torch::empty_like(normals);
  loss_call("grpg_normal_loss_backward", [&](void* stream) {
    return grpg_normal_loss_backward(in.H, in.W, normals.data_ptr<float>(), mono.data_ptr<float>(),
                                     wvt.data_ptr<float>(), in.rs, in.cs, in.mask, in.sky, normalize ? 1 : 0,
                                     (int)top_rows, g.data_ptr<float>(), ws.data_ptr(), grad.data_ptr<float>(), stream);
  });
  return grad;
}

// Fused scale-flatten / opacity-sparse regularisers (gaussianrpg_amd/loss.py).  scaling: empty (term off) or a
// contiguous float32 [N,3]; opacities: one contiguous float32 [N_i,1] or [N_i] tensor per model; radii: contiguous
// int32 of sum N_i elements.  A term is on when its lambda is > 0.  Returns (stats [4], workspace).
namespace {
struct RegIn {
  torch::Device dev = torch::kCPU;
  const float* scaling = nullptr;
  int64_t n_scaling = 0, total = 0;
  std::vector<grpg_reg_segment> segs;
  const int* radii = nullptr;
};

RegIn reg_args(const char* fn, const torch::Tensor& scaling, const std::vector<torch::Tensor>& opacities,
               const torch::Tensor& radii, const double lam_scale, const double lam_opacity) {
  RegIn in;
  bool any = false;
  auto on_device = [&](const torch::Tensor& t, const char* what) {
    TORCH_CHECK(t.defined(), fn, ": undefined ", what);
    TORCH_CHECK(t.is_cuda(), fn, ": ", what, " must live on a ROCm/HIP device (no CPU path)");
    TORCH_CHECK(!any || t.device() == in.dev, fn, ": tensors on different devices");
    in.dev = t.device();
    any = true;
  };
  if (lam_scale > 0) {
    on_device(scaling, "scaling");
    TORCH_CHECK(scaling.scalar_type() == torch::kFloat32 && scaling.dim() == 2 && scaling.size(1) == 3 &&
                    scaling.is_contiguous(), fn, ": scaling must be a contiguous float32 [N,3] tensor");
    in.n_scaling = scaling.size(0);
    in.scaling = in.n_scaling ? scaling.data_ptr<float>() : nullptr;
  }
  if (lam_opacity > 0) {
    on_device(radii, "radii");
    TORCH_CHECK(radii.scalar_type() == torch::kInt32 && radii.dim() == 1 && radii.is_contiguous(), fn,
                ": radii must be a contiguous int32 [sum N_i] tensor");
    for (const torch::Tensor& t : opacities) {
      on_device(t, "opacity");
      TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.is_contiguous() &&
                      (t.dim() == 1 || (t.dim() == 2 && t.size(1) == 1)),
                  fn, ": every opacity tensor must be a contiguous float32 [N_i,1] or [N_i]");
      in.segs.push_back(grpg_reg_segment{t.numel() ? t.data_ptr<float>() : nullptr, nullptr, t.numel()});
      in.total += t.numel();
    }
    TORCH_CHECK(radii.numel() == in.total, fn, ": radii has ", radii.numel(), " elements, the opacities ", in.total);
    in.radii = in.total ? radii.data_ptr<int>() : nullptr;
  }
  TORCH_CHECK(any, fn, ": no term is on");
  return in;
}
}  // namespace

std::tuple<torch::Tensor, torch::Tensor> RegLossForward(const torch::Tensor& scaling, const bool scale_activated,
                                                        const std::vector<torch::Tensor>& opacities,
                                                        const bool opacity_activated, const torch::Tensor& radii,
                                                        const double lam_scale, const double lam_opacity) {
  RegIn in = reg_args("reg_loss_forward", scaling, opacities, radii, lam_scale, lam_opacity);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.dev);
  torch::Tensor stats = torch::empty({4}, torch::TensorOptions().dtype(torch::kFloat32).device(in.dev));
  torch::Tensor ws = loss_workspace(grpg_reg_loss_workspace_bytes((int)in.segs.size()), in.dev);
  loss_call("grpg_reg_loss_forward", [&](void* stream) {
    return grpg_reg_loss_forward(in.scaling, in.n_scaling, scale_activated ? 1 : 0, in.segs.data(), (int)in.segs.size(),
                                 opacity_activated ? 1 : 0, in.radii, in.total, (float)lam_scale, (float)lam_opacity,
                                 stats.data_ptr<float>(), ws.data_ptr(), stream);
  });
  return std::make_tuple(stats, ws);
}

// Returns (grad_scaling: the shape of scaling, or empty when not wanted; one gradient per opacity tensor, of its
// shape, or empty where want_opacity[i] is false).
std::tuple<torch::Tensor, std::vector<torch::Tensor>> RegLossBackward(
    const torch::Tensor& scaling, const bool scale_activated, const std::vector<torch::Tensor>& opacities,
    const bool opacity_activated, const torch::Tensor& radii, const double lam_scale, const double lam_opacity,
    const torch::Tensor& grad_stats, const torch::Tensor& ws, const bool want_scale,
    const std::vector<bool>& want_opacity) {
  RegIn in = reg_args("reg_loss_backward", scaling, opacities, radii, lam_scale, lam_opacity);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(in.dev);
  TORCH_CHECK(ws.device() == in.dev && ws.scalar_type() == torch::kByte && ws.is_contiguous() &&
                  (size_t)ws.numel() == grpg_reg_loss_workspace_bytes((int)in.segs.size()),
              "reg_loss_backward: workspace does not match");
  TORCH_CHECK(lam_opacity <= 0 || want_opacity.size() == opacities.size(),
              "reg_loss_backward: one want_opacity flag per opacity tensor");
  const torch::Tensor g = loss_grad_stats(grad_stats, in.dev, 4, "reg_loss_backward: grad_stats must have 4 elements");
  auto fopts = torch::TensorOptions().dtype(torch::kFloat32).device(in.dev);
  torch::Tensor gs = (want_scale && lam_scale > 0) ? torch::empty_like(scaling) : torch::empty({0}, fopts);
  std::vector<torch::Tensor> go;
  for (size_t i = 0; i < in.segs.size(); i++) {
    go.push_back(want_opacity[i] ? torch::empty_like(opacities[i]) : torch::empty({0}, fopts));
    if (want_opacity[i] && in.segs[i].n) in.segs[i].grad_opacity = go[i].data_ptr<float>();
  }
  loss_call("grpg_reg_loss_backward", [&](void* stream) {
    return grpg_reg_loss_backward(in.scaling, in.n_scaling, scale_activated ? 1 : 0, in.segs.data(),
                                  (int)in.segs.size(), opacity_activated ? 1 : 0, in.radii, in.total, (float)lam_scale,
                                  (float)lam_opacity, g.data_ptr<float>(), ws.data_ptr(),
                                  gs.numel() ? gs.data_ptr<float>() : nullptr, stream);
  });
  return std::make_tuple(gs, go);
}

// PSNR (gaussianrpg_amd/loss.py).  img1 / img2: contiguous float32 [C,H,W]; mask: empty or contiguous uint8 of H*W
// elements.  Returns stats [2]: psnr, mse.
torch::Tensor PsnrForward(const torch::Tensor& img1, const torch::Tensor& img2, const torch::Tensor& mask) {
  TORCH_CHECK(img1.defined() && img2.defined(), "psnr: undefined tensor");
  TORCH_CHECK(img1.is_cuda() && img2.is_cuda(), "psnr: images must live on a ROCm/HIP device (no CPU path)");
  TORCH_CHECK(img1.device() == img2.device(), "psnr: images on different devices");
  TORCH_CHECK(img1.scalar_type() == torch::kFloat32 && img2.scalar_type() == torch::kFloat32 && img1.dim() == 3 &&
                  img1.sizes() == img2.sizes() && img1.is_contiguous() && img2.is_contiguous(),
              "psnr: images must be two contiguous float32 [C,H,W] tensors of one shape");
  const int64_t C = img1.size(0), H = img1.size(1), W = img1.size(2);
  TORCH_CHECK(C >= 1 && C <= 0x7FFFFFFFll && H > 0 && W > 0 && H * W <= 0x7FFFFFFFll,
              "psnr: C, H and W must be positive with H*W < 2^31");
  const unsigned char* pm = nullptr;
  if (mask.defined() && mask.numel() > 0) {
    TORCH_CHECK(mask.is_cuda() && mask.device() == img1.device() && mask.scalar_type() == torch::kUInt8 &&
                    mask.is_contiguous() && mask.numel() == H * W,
                "psnr: mask must be a contiguous uint8 plane of H*W elements on the images' device");
    pm = mask.data_ptr<uint8_t>();
  }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(img1.device());
  torch::Tensor stats = torch::empty({2}, torch::TensorOptions().dtype(torch::kFloat32).device(img1.device()));
  torch::Tensor ws = loss_workspace(grpg_psnr_workspace_bytes(), img1.device());
  loss_call("grpg_psnr_forward", [&](void* stream) {
    return grpg_psnr_forward((int)C, (int)H, (int)W, img1.data_ptr<float>(), img2.data_ptr<float>(), pm,
                             stats.data_ptr<float>(), ws.data_ptr(), stream);
  });
  return stats;
}

// The tail of the training iteration (gaussianrpg_amd/optim.py): optimizer.step() of every tensor of every
// optimizer in one launch, and the densification statistics of every model in one launch.
namespace {
float* optim_f(const torch::Tensor& t, const torch::Device& dev, const int64_t numel, const char* fn,
               const char* what) {
  TORCH_CHECK(t.defined(), fn, ": undefined ", what);
  TORCH_CHECK(t.is_cuda(), fn, ": ", what, " must live on a ROCm/HIP device (no CPU path)");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, fn, ": ", what, " must be float32");
  TORCH_CHECK(t.device() == dev, fn, ": tensors on different devices");
  TORCH_CHECK(t.is_contiguous(), fn, ": ", what, " must be contiguous");
  TORCH_CHECK(t.numel() == numel, fn, ": ", what, " has ", t.numel(), " elements, expected ", numel);
  return numel ? t.data_ptr<float>() : nullptr;
}
}  // namespace

// coef: CPU float32 [S, 6] = (step_size, bc2_sqrt, beta2, 1 - beta1, 1 - beta2, eps) per segment.
void AdamStep(const std::vector<torch::Tensor>& params, const std::vector<torch::Tensor>& grads,
              const std::vector<torch::Tensor>& exp_avgs, const std::vector<torch::Tensor>& exp_avg_sqs,
              const torch::Tensor& coef) {
  const size_t S = params.size();
  TORCH_CHECK(grads.size() == S && exp_avgs.size() == S && exp_avg_sqs.size() == S,
              "adam_step: the four tensor lists must have one entry per segment");
  TORCH_CHECK(coef.device().is_cpu() && coef.scalar_type() == torch::kFloat32 && coef.is_contiguous() &&
                  coef.dim() == 2 && (size_t)coef.size(0) == S && coef.size(1) == 6,
              "adam_step: coef must be a contiguous CPU float32 [segments, 6] tensor");
  if (S == 0) return;
  TORCH_CHECK(params[0].defined() && params[0].is_cuda(),
              "adam_step: param must live on a ROCm/HIP device (no CPU path)");
  const torch::Device dev = params[0].device();
  std::vector<grpg_adam_segment> segs(S);
  const float* c = coef.data_ptr<float>();
  for (size_t i = 0; i < S; i++) {
    grpg_adam_segment& g = segs[i];
    const int64_t n = params[i].defined() ? params[i].numel() : 0;
    g.param = optim_f(params[i], dev, n, "adam_step", "param");
    g.grad = optim_f(grads[i], dev, n, "adam_step", "grad");
    g.exp_avg = optim_f(exp_avgs[i], dev, n, "adam_step", "exp_avg");
    g.exp_avg_sq = optim_f(exp_avg_sqs[i], dev, n, "adam_step", "exp_avg_sq");
    g.n = n;
    g.step_size = c[6 * i]; g.bc2_sqrt = c[6 * i + 1]; g.beta2 = c[6 * i + 2];
    g.one_minus_beta1 = c[6 * i + 3]; g.one_minus_beta2 = c[6 * i + 4]; g.eps = c[6 * i + 5];
  }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  torch::Tensor table = torch::empty({0}, torch::TensorOptions().dtype(torch::kByte).device(dev));
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int rc = grpg_adam_step(segs.data(), (int)S, resize_blob, &table, (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_adam_step", rc);
  for (size_t i = 0; i < S; i++) {     // written in place behind autograd's back: tell the version counters
    if (!segs[i].n) continue;
    params[i].unsafeGetTensorImpl()->bump_version();
    exp_avgs[i].unsafeGetTensorImpl()->bump_version();
    exp_avg_sqs[i].unsafeGetTensorImpl()->bump_version();
  }
}

// grad [P,3] float32, radii [P] int32, ranges: CPU int64 [R,2] half-open; per range accum [n,2], denom [n,1] or
// [n], max_radii [n], updated in place.
void DensifyStats(const torch::Tensor& grad, const torch::Tensor& radii, const torch::Tensor& ranges,
                  const std::vector<torch::Tensor>& accum, const std::vector<torch::Tensor>& denom,
                  const std::vector<torch::Tensor>& max_radii) {
  TORCH_CHECK(grad.defined() && grad.is_cuda(),
              "densify_stats: grad must live on a ROCm/HIP device (no CPU path)");
  TORCH_CHECK(grad.scalar_type() == torch::kFloat32 && grad.dim() == 2 && grad.size(1) == 3 && grad.is_contiguous(),
              "densify_stats: grad must be a contiguous float32 [P,3] tensor");
  const int64_t P = grad.size(0);
  TORCH_CHECK(P <= 0x7FFFFFFFll, "densify_stats: P must be < 2^31");
  const torch::Device dev = grad.device();
  TORCH_CHECK(radii.is_cuda() && radii.device() == dev, "densify_stats: radii must live on grad's device (no CPU path)");
  TORCH_CHECK(radii.scalar_type() == torch::kInt32 && radii.numel() == P && radii.is_contiguous(),
              "densify_stats: radii must be a contiguous int32 [P] tensor");
  const size_t R = accum.size();
  TORCH_CHECK(denom.size() == R && max_radii.size() == R, "densify_stats: one accum / denom / max_radii2D per range");
  TORCH_CHECK(ranges.device().is_cpu() && ranges.scalar_type() == torch::kInt64 && ranges.is_contiguous() &&
                  ranges.dim() == 2 && (size_t)ranges.size(0) == R && ranges.size(1) == 2,
              "densify_stats: ranges must be a contiguous CPU int64 [ranges, 2] tensor");
  std::vector<grpg_range> rs(R);
  std::vector<float*> pa(R), pd(R), pm(R);
  const int64_t* rp = ranges.data_ptr<int64_t>();
  for (size_t i = 0; i < R; i++) {
    const int64_t s = rp[2 * i], e = rp[2 * i + 1];
    TORCH_CHECK(0 <= s && s <= e && e <= P, "densify_stats: range [", s, ", ", e, ") outside [0, ", P, "]");
    rs[i] = grpg_range{(int)s, (int)e};
    const int64_t n = e - s;
    TORCH_CHECK(accum[i].defined() && accum[i].dim() == 2 && accum[i].size(1) == 2,
                "densify_stats: accum must be [n,2]");
    pa[i] = optim_f(accum[i], dev, 2 * n, "densify_stats", "accum");
    pd[i] = optim_f(denom[i], dev, n, "densify_stats", "denom");
    pm[i] = optim_f(max_radii[i], dev, n, "densify_stats", "max_radii2D");
  }
  if (P == 0 || R == 0) return;
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  torch::Tensor table = torch::empty({0}, torch::TensorOptions().dtype(torch::kByte).device(dev));
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int rc = grpg_densify_stats((int)P, grad.data_ptr<float>(), radii.data_ptr<int>(), rs.data(), (int)R,
                                    pa.data(), pd.data(), pm.data(), resize_blob, &table, (void*)stream);
  if (rc != GRPG_OK) raise_abi_error("grpg_densify_stats", rc);
  for (size_t i = 0; i < R; i++) {
    if (rs[i].end == rs[i].start) continue;
    accum[i].unsafeGetTensorImpl()->bump_version();
    denom[i].unsafeGetTensorImpl()->bump_version();
    max_radii[i].unsafeGetTensorImpl()->bump_version();
  }
}

// densify_and_prune of every model (gaussianrpg_amd/optim.py): plan (classify + scan, the call's one host wait), the
// outputs from torch's allocator, apply.  params[m][t]: float32 [P_m, ...]; has_state[m][t] says whether
// exp_avgs[m][t] / exp_avg_sqs[m][t] are the tensor's moments (otherwise they are ignored); special: CPU int64 [M,4]
// = the indices of xyz, opacity, scaling, rotation; rules: CPU float64 [M,19] = grad_column, max_grad, percent_dense,
// extent, min_opacity, prune_big, percent_big_ws, has_sphere, centre[3], radius, has_box, box_min[3], box_max[3].
// Returns per model (params, exp_avgs, exp_avg_sqs, accum [n,2], denom [n,1], max_radii2D [n], src_index [n]) and the
// counts as a CPU int64 [M,10] tensor (grpg_densify_counts).
using DensifyModelOut = std::tuple<std::vector<torch::Tensor>, std::vector<torch::Tensor>, std::vector<torch::Tensor>,
                                   torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>;
std::tuple<std::vector<DensifyModelOut>, torch::Tensor> DensifyAndPrune(
    const std::vector<std::vector<torch::Tensor>>& params, const std::vector<std::vector<torch::Tensor>>& exp_avgs,
    const std::vector<std::vector<torch::Tensor>>& exp_avg_sqs, const std::vector<std::vector<int64_t>>& has_state,
    const std::vector<torch::Tensor>& accum, const std::vector<torch::Tensor>& denom,
    const std::vector<torch::Tensor>& split_noise, const std::vector<torch::Tensor>& box_noise,
    const torch::Tensor& special, const torch::Tensor& rules) {
  const size_t M = params.size();
  TORCH_CHECK(exp_avgs.size() == M && exp_avg_sqs.size() == M && has_state.size() == M && accum.size() == M &&
                  denom.size() == M && split_noise.size() == M && box_noise.size() == M,
              "densify_and_prune: one entry per model in every list");
  TORCH_CHECK(special.device().is_cpu() && special.scalar_type() == torch::kInt64 && special.is_contiguous() &&
                  special.dim() == 2 && (size_t)special.size(0) == M && special.size(1) == 4,
              "densify_and_prune: special must be a contiguous CPU int64 [models, 4] tensor");
  TORCH_CHECK(rules.device().is_cpu() && rules.scalar_type() == torch::kFloat64 && rules.is_contiguous() &&
                  rules.dim() == 2 && (size_t)rules.size(0) == M && rules.size(1) == 19,
              "densify_and_prune: rules must be a contiguous CPU float64 [models, 19] tensor");
  torch::Tensor counts = torch::zeros({(long long)M, 10}, torch::TensorOptions().dtype(torch::kInt64));
  static_assert(sizeof(grpg_densify_counts) == 10 * sizeof(int64_t), "counts travel as an int64 [M,10] tensor");
  std::vector<DensifyModelOut> result(M);
  if (M == 0) return std::make_tuple(result, counts);
  TORCH_CHECK(accum[0].defined() && accum[0].is_cuda(),
              "densify_and_prune: tensors must live on a ROCm/HIP device (no CPU path)");
  const torch::Device dev = accum[0].device();
  std::vector<grpg_densify_model> models(M);
  std::vector<long long> rows(M);
  const int64_t* sp = special.data_ptr<int64_t>();
  const double* ru = rules.data_ptr<double>();
  for (size_t m = 0; m < M; m++) {
    grpg_densify_model& g = models[m];
    g = grpg_densify_model{};
    const size_t T = params[m].size();
    TORCH_CHECK(T >= 1 && T <= (size_t)GRPG_DENSIFY_MAX_TENSORS, "densify_and_prune: a model has 1 to ",
                GRPG_DENSIFY_MAX_TENSORS, " tensors");
    TORCH_CHECK(exp_avgs[m].size() == T && exp_avg_sqs[m].size() == T && has_state[m].size() == T,
                "densify_and_prune: one moment pair and one has_state flag per tensor");
    TORCH_CHECK(accum[m].defined() && accum[m].dim() == 2 && accum[m].size(1) == 2,
                "densify_and_prune: xyz_gradient_accum must be [P,2]");
    const int64_t P = accum[m].size(0);
    g.P = rows[m] = P;
    g.num_tensors = (int)T;
    for (size_t t = 0; t < T; t++) {
      const torch::Tensor& p = params[m][t];
      TORCH_CHECK(p.defined() && p.dim() >= 1 && p.size(0) == P, "densify_and_prune: every tensor of a model has P rows");
      int64_t w = 1;
      for (int64_t k = 1; k < p.dim(); k++) w *= p.size(k);
      TORCH_CHECK(w <= 0x7FFFFFFFll, "densify_and_prune: row too wide");
      grpg_densify_tensor& D = g.tensors[t];
      D.width = (int)w;
      D.param = optim_f(p, dev, P * w, "densify_and_prune", "param");
      if (has_state[m][t]) {
        TORCH_CHECK(exp_avgs[m][t].defined() && exp_avgs[m][t].sizes() == p.sizes() &&
                        exp_avg_sqs[m][t].defined() && exp_avg_sqs[m][t].sizes() == p.sizes(),
                    "densify_and_prune: moments must have their parameter's shape");
        D.exp_avg = optim_f(exp_avgs[m][t], dev, P * w, "densify_and_prune", "exp_avg");
        D.exp_avg_sq = optim_f(exp_avg_sqs[m][t], dev, P * w, "densify_and_prune", "exp_avg_sq");
      }
    }
    g.xyz_index = (int)sp[4 * m]; g.opacity_index = (int)sp[4 * m + 1];
    g.scaling_index = (int)sp[4 * m + 2]; g.rotation_index = (int)sp[4 * m + 3];
    g.xyz_gradient_accum = optim_f(accum[m], dev, 2 * P, "densify_and_prune", "xyz_gradient_accum");
    g.denom = optim_f(denom[m], dev, P, "densify_and_prune", "denom");
    g.split_noise = optim_f(split_noise[m], dev, 6 * P, "densify_and_prune", "split_noise");
    const double* r = ru + 19 * m;
    g.grad_column = (int)r[0]; g.max_grad = (float)r[1]; g.percent_dense = (float)r[2]; g.extent = (float)r[3];
    g.min_opacity = (float)r[4]; g.prune_big = r[5] != 0.0; g.percent_big_ws = (float)r[6];
    g.has_sphere = r[7] != 0.0;
    for (int k = 0; k < 3; k++) {
      g.sphere_center[k] = (float)r[8 + k];
      g.box_min[k] = (float)r[13 + k];
      g.box_max[k] = (float)r[16 + k];
    }
    g.sphere_radius = (float)r[11];
    g.has_box = r[12] != 0.0;
    if (g.has_box && g.prune_big)
      g.box_noise = optim_f(box_noise[m], dev, 24 * P, "densify_and_prune", "box_noise");
  }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  const auto bytes_opt = torch::TensorOptions().dtype(torch::kByte).device(dev);
  const auto f_opt = torch::TensorOptions().dtype(torch::kFloat32).device(dev);
  torch::Tensor ws = loss_workspace(grpg_densify_workspace_bytes(rows.data(), (int)M), dev);
  torch::Tensor table = torch::empty({0}, bytes_opt), table2 = torch::empty({0}, bytes_opt);
  grpg_densify_counts* cnt = reinterpret_cast<grpg_densify_counts*>(counts.data_ptr<int64_t>());
  loss_call("grpg_densify_plan", [&](void* stream) {
    return grpg_densify_plan(models.data(), (int)M, ws.data_ptr(), cnt, resize_blob, &table, stream);
  });
  std::vector<grpg_densify_output> outs(M);
  for (size_t m = 0; m < M; m++) {
    grpg_densify_output& o = outs[m];
    o = grpg_densify_output{};
    const int64_t n = cnt[m].n_out;
    TORCH_CHECK(n >= 0 && n <= 3 * rows[m], "densify_and_prune: the plan returned an impossible row count");
    o.n_out = n;
    auto& [np, nm, nv, na, nd, nr, ni] = result[m];
    for (size_t t = 0; t < params[m].size(); t++) {
      std::vector<int64_t> shape = params[m][t].sizes().vec();
      shape[0] = n;
      np.push_back(torch::empty(shape, f_opt));
      nm.push_back(has_state[m][t] ? torch::empty(shape, f_opt) : torch::Tensor(torch::empty({0}, f_opt)));
      nv.push_back(has_state[m][t] ? torch::empty(shape, f_opt) : torch::Tensor(torch::empty({0}, f_opt)));
      const bool live = np.back().numel() > 0;
      o.tensors[t].param = live ? np.back().data_ptr<float>() : nullptr;
      if (has_state[m][t] && live) {
        o.tensors[t].exp_avg = nm.back().data_ptr<float>();
        o.tensors[t].exp_avg_sq = nv.back().data_ptr<float>();
      }
    }
    na = torch::empty({n, 2}, f_opt);
    nd = torch::empty({n, 1}, f_opt);
    nr = torch::empty({n}, f_opt);
    ni = torch::empty({n}, f_opt.dtype(torch::kInt32));
    if (n > 0) {
      o.xyz_gradient_accum = na.data_ptr<float>();
      o.denom = nd.data_ptr<float>();
      o.max_radii2D = nr.data_ptr<float>();
      o.src_index = ni.data_ptr<int>();
    }
  }
  loss_call("grpg_densify_apply", [&](void* stream) {
    return grpg_densify_apply(models.data(), (int)M, ws.data_ptr(), outs.data(), resize_blob, &table2, stream);
  });
  return std::make_tuple(result, counts);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rasterize_gaussians", &RasterizeGaussians);
  m.def("rasterize_gaussians_eval", &RasterizeGaussiansEval);
  m.def("rasterize_gaussians_eval_deferred", &RasterizeGaussiansEvalDeferred);
  m.def("rasterize_gaussians_layers", &RasterizeGaussiansLayers);
  m.def("frame_status", &FrameStatus, pybind11::arg("ticket"), pybind11::arg("wait") = true);
  m.def("distCUDA2", &distCUDA2);
  m.def("ssim_forward", &SsimForward);     // (stats [4+B], saved partials)
  m.def("ssim_backward", &SsimBackward);
  m.def("aux_loss_forward", &AuxLossForward);    // (stats [9], workspace)
  m.def("aux_loss_backward", &AuxLossBackward);
  m.def("semantic_ce_forward", &SemanticCeForward);    // (stats [4], workspace, labels)
  m.def("semantic_ce_backward", &SemanticCeBackward, pybind11::arg("semantic"), pybind11::arg("target"),
        pybind11::arg("mode"), pybind11::arg("grad_stats"), pybind11::arg("workspace"),
        pybind11::arg("grad_out") = pybind11::none());
  m.def("normal_loss_forward", &NormalLossForward);    // (stats [4], workspace)
  m.def("normal_loss_backward", &NormalLossBackward);
  m.def("reg_loss_forward", &RegLossForward);          // (stats [4], workspace)
  m.def("reg_loss_backward", &RegLossBackward);        // (grad_scaling, [grad_opacity per model])
  m.def("psnr_forward", &PsnrForward);                 // stats [2]: psnr, mse
  m.def("adam_step", &AdamStep);            // in place: params, exp_avgs, exp_avg_sqs
  m.def("densify_stats", &DensifyStats);    // in place: accum, denom, max_radii2D
  m.def("densify_and_prune", &DensifyAndPrune);   // ([per model outputs], counts [M,10])
  m.def("rasterize_gaussians_backward", &RasterizeGaussiansBackward);
  m.def("rasterize_gaussians_backward_lean", &RasterizeGaussiansBackwardLean);
  m.def("mark_visible", &markVisible);
  m.def("rasterize_gaussians_filter", &RasterizeGaussiansFilter);
  // additions (not in the reference module)
  m.def("debug_export", &DebugExport);
  m.def("rasterize_gaussians_composed", &RasterizeGaussiansComposed, pybind11::arg("bg"), pybind11::arg("xyz"),
        pybind11::arg("scaling"), pybind11::arg("rotation"), pybind11::arg("opacity"),
        pybind11::arg("features_dc"), pybind11::arg("features_rest"), pybind11::arg("flip"), pybind11::arg("poses"),
        pybind11::arg("idft"), pybind11::arg("scale_modifier"), pybind11::arg("viewmatrix"),
        pybind11::arg("projmatrix"), pybind11::arg("tan_fovx"), pybind11::arg("tan_fovy"),
        pybind11::arg("image_height"), pybind11::arg("image_width"), pybind11::arg("degree"),
        pybind11::arg("campos"), pybind11::arg("debug"), pybind11::arg("for_backward") = false);
  m.def("rasterize_gaussians_composed_backward", &RasterizeGaussiansComposedBackward);
  m.def("rasterize_gaussians_composed_objects_backward", &RasterizeGaussiansComposedObjectsBackward);
  m.def("object_alpha_forward", &ObjectAlphaForward);   // (alpha_object [1,H,W], workspace)
  m.def("rasterize_gaussians_composed_layers", &RasterizeGaussiansComposedLayers);
  // (the arguments are named for the sake of the one default: affine, the colour correction inside the epilogue)
  m.def("rasterize_gaussians_frame", &RasterizeGaussiansFrame,
        pybind11::arg("background"), pybind11::arg("layer_background"), pybind11::arg("layer_class"),
        pybind11::arg("means3D"), pybind11::arg("colors"), pybind11::arg("opacity"), pybind11::arg("scales"),
        pybind11::arg("rotations"), pybind11::arg("scale_modifier"), pybind11::arg("cov3D_precomp"),
        pybind11::arg("viewmatrix"), pybind11::arg("projmatrix"), pybind11::arg("tan_fovx"),
        pybind11::arg("tan_fovy"), pybind11::arg("image_height"), pybind11::arg("image_width"), pybind11::arg("sh"),
        pybind11::arg("degree"), pybind11::arg("campos"), pybind11::arg("debug"), pybind11::arg("sky_cube"),
        pybind11::arg("ray_matrix"), pybind11::arg("sky_fill"), pybind11::arg("clamp"), pybind11::arg("want_planes"),
        pybind11::arg("want_rgb8"), pybind11::arg("truncate"), pybind11::arg("out_rgb8"),
        pybind11::arg("affine") = pybind11::none());
  m.def("rasterize_gaussians_composed_frame", &RasterizeGaussiansComposedFrame,
        pybind11::arg("background"), pybind11::arg("layer_background"), pybind11::arg("object_model"),
        pybind11::arg("layered"), pybind11::arg("xyz"), pybind11::arg("scaling"), pybind11::arg("rotation"),
        pybind11::arg("opacity"), pybind11::arg("features_dc"), pybind11::arg("features_rest"), pybind11::arg("flip"),
        pybind11::arg("poses"), pybind11::arg("idft"), pybind11::arg("scale_modifier"), pybind11::arg("viewmatrix"),
        pybind11::arg("projmatrix"), pybind11::arg("tan_fovx"), pybind11::arg("tan_fovy"),
        pybind11::arg("image_height"), pybind11::arg("image_width"), pybind11::arg("degree"), pybind11::arg("campos"),
        pybind11::arg("debug"), pybind11::arg("sky_cube"), pybind11::arg("ray_matrix"), pybind11::arg("sky_fill"),
        pybind11::arg("clamp"), pybind11::arg("want_planes"), pybind11::arg("want_rgb8"), pybind11::arg("truncate"),
        pybind11::arg("out_rgb8"),
        pybind11::arg("affine") = pybind11::none());
  m.def("compose", &Compose);
  m.def("compose_features", &ComposeFeatures);
  m.def("compose_features_backward", &ComposeFeaturesBackward);
  m.def("rasterize_gaussians_composed_features", &RasterizeGaussiansComposedFeatures);
  // the baked segment tables of a pose tape and the frame call on them (session.py FrameSession)
  pybind11::class_<FrameTables, std::shared_ptr<FrameTables>>(m, "FrameTables")
      .def_property_readonly("rows", [](const FrameTables& t) { return t.rows; })   // uint8 [R * 144], device
      .def_property_readonly("first", [](const FrameTables& t) { return t.first; })
      .def_property_readonly("num_gaussians", [](const FrameTables& t) { return t.P; })
      .def("__len__", &FrameTables::num_frames);
  m.def("bake_frame_tables", &BakeFrameTables);
  m.def("rasterize_gaussians_bound_frame", &RasterizeGaussiansBoundFrame);
  m.def("frame_tables_bytes", [](long long rows) { return grpg_frame_tables_bytes(rows); });
  m.def("bind_frame_table", [](const torch::Tensor& rows, int num_segments, int P) {   // the tests' refusals
    return grpg_bind_frame_table(rows.data_ptr(), num_segments, P);
  });
  m.def("frame_tables_bound", []() { return grpg_frame_tables_bound(); });
  m.def("sky_composite", &SkyComposite, pybind11::arg("cube"), pybind11::arg("ray_matrix"),
        pybind11::arg("fill"), pybind11::arg("clamp_out"), pybind11::arg("rgb"), pybind11::arg("acc"),
        pybind11::arg("height"), pybind11::arg("width"), pybind11::arg("want_sky"),
        pybind11::arg("mask") = pybind11::none(), pybind11::arg("jitter") = pybind11::none());
  m.def("sky_backward", &SkyBackward, pybind11::arg("cube"), pybind11::arg("ray_matrix"),
        pybind11::arg("fill"), pybind11::arg("acc"), pybind11::arg("grad_rgb"),
        pybind11::arg("mask") = pybind11::none(), pybind11::arg("jitter") = pybind11::none());
  m.def("pack_u8", &PackU8, pybind11::arg("color"), pybind11::arg("out") = pybind11::none());
  m.def("pack_hwc", &PackHWC);
  // colour correction of the frame (appearance.py): (planes, rgb8) / (grad_x, grad_affine)
  m.def("color_correct", &ColorCorrect, pybind11::arg("rgb"), pybind11::arg("affine"), pybind11::arg("clamp") = false,
        pybind11::arg("planes") = true, pybind11::arg("rgb8") = false, pybind11::arg("truncate") = true,
        pybind11::arg("out") = pybind11::none(), pybind11::arg("cube") = pybind11::none(),
        pybind11::arg("ray_matrix") = pybind11::none(), pybind11::arg("fill") = 0.0,
        pybind11::arg("acc") = pybind11::none(), pybind11::arg("mask") = pybind11::none(),
        pybind11::arg("jitter") = pybind11::none());
  m.def("color_correct_backward", &ColorCorrectBackward, pybind11::arg("rgb"), pybind11::arg("affine"),
        pybind11::arg("grad"), pybind11::arg("need_x") = true, pybind11::arg("need_affine") = true,
        pybind11::arg("cube") = pybind11::none(), pybind11::arg("ray_matrix") = pybind11::none(),
        pybind11::arg("fill") = 0.0, pybind11::arg("acc") = pybind11::none(), pybind11::arg("mask") = pybind11::none(),
        pybind11::arg("jitter") = pybind11::none());
  m.def("color_correct_workspace_bytes", [](int H, int W) { return grpg_color_correct_workspace_bytes(W, H); });
  // colour correction, use_mlp variant (appearance.py ColorCorrectionMLP): (affine, x, reg, hidden) / (gw x 8, gb x 8)
  m.def("color_mlp_forward", &ColorMlpForward, pybind11::arg("weights"), pybind11::arg("biases"),
        pybind11::arg("ego_pose"), pybind11::arg("extrinsic"), pybind11::arg("want_reg") = true,
        pybind11::arg("want_hidden") = true);
  m.def("color_mlp_backward", &ColorMlpBackward, pybind11::arg("weights"), pybind11::arg("biases"), pybind11::arg("x"),
        pybind11::arg("hidden"), pybind11::arg("affine"), pybind11::arg("grad_affine") = pybind11::none(),
        pybind11::arg("grad_reg") = pybind11::none());
  // pose correction of the background (pose_correction.py): (xyz', rotation') / (g_xyz, g_rotation, g_rot, g_trans)
  m.def("pose_correct", &PoseCorrect, pybind11::arg("xyz"), pybind11::arg("rotation"), pybind11::arg("rot"),
        pybind11::arg("trans"));
  m.def("pose_correct_backward", &PoseCorrectBackward, pybind11::arg("xyz"), pybind11::arg("rotation"),
        pybind11::arg("rot"), pybind11::arg("trans"), pybind11::arg("grad_xyz"), pybind11::arg("grad_rotation"),
        pybind11::arg("need_xyz") = true, pybind11::arg("need_rotation") = true, pybind11::arg("need_rot") = true,
        pybind11::arg("need_trans") = true);
  m.def("pose_correct_workspace_bytes", [](int n) { return grpg_pose_correct_workspace_bytes(n); });
  // the frame's pose table with the background's row behind the actors' (pose_correction.py)
  m.def("pose_rows", &PoseRowsForward, pybind11::arg("rot"), pybind11::arg("trans"), pybind11::arg("corr_rots"),
        pybind11::arg("corr_trans"), pybind11::arg("id"));
  m.def("pose_rows_backward", &PoseRowsBackward, pybind11::arg("grad_rot"), pybind11::arg("grad_trans"),
        pybind11::arg("n"), pybind11::arg("id"));
  // frame -> detector input (perception.py)
  m.def("letterbox_geometry", &LetterboxGeometry, pybind11::arg("height"), pybind11::arg("width"),
        pybind11::arg("new_h_req"), pybind11::arg("new_w_req"), pybind11::arg("auto_pad") = true,
        pybind11::arg("scale_fill") = false, pybind11::arg("scaleup") = true, pybind11::arg("stride") = 32);
  m.def("letterbox_tables", &LetterboxTables);   // (x_table [new_w,2], y_table [new_h,2]), host int32
  m.def("letterbox_rgb8", &LetterboxRgb8, pybind11::arg("frame"), pybind11::arg("geometry"),
        pybind11::arg("x_table") = pybind11::none(), pybind11::arg("y_table") = pybind11::none(),
        pybind11::arg("reverse_channels") = true, pybind11::arg("out") = pybind11::none(),
        pybind11::arg("half") = false);
  m.def("letterbox_planes", &LetterboxPlanes, pybind11::arg("frame"), pybind11::arg("geometry"),
        pybind11::arg("x_table") = pybind11::none(), pybind11::arg("y_table") = pybind11::none(),
        pybind11::arg("reverse_channels") = true, pybind11::arg("truncate") = true,
        pybind11::arg("out") = pybind11::none(), pybind11::arg("half") = false);
  // detector output -> detections (perception.py): (det [bs,max_det,6], count [bs])
  m.def("nms_detections", &NmsDetections, pybind11::arg("prediction"), pybind11::arg("conf_thres") = 0.25,
        pybind11::arg("iou_thres") = 0.45, pybind11::arg("class_allow") = pybind11::none(),
        pybind11::arg("agnostic") = false, pybind11::arg("max_det") = 300, pybind11::arg("max_nms") = 30000,
        pybind11::arg("max_wh") = 7680.0, pybind11::arg("frame_map") = std::vector<double>(),
        pybind11::arg("det_out") = pybind11::none(), pybind11::arg("count_out") = pybind11::none());
  m.def("nms_workspace_bytes", [](int bs, int N) { return grpg_nms_workspace_bytes(bs, N); });
  // detector head -> prediction [bs,N,5+nc] / detections (perception.py)
  m.def("detect_decode", &DetectDecode, pybind11::arg("heads"), pybind11::arg("anchor_grid"), pybind11::arg("stride"),
        pybind11::arg("na"), pybind11::arg("nc"), pybind11::arg("out") = pybind11::none());
  m.def("detect_detections", &DetectDetections, pybind11::arg("heads"), pybind11::arg("anchor_grid"),
        pybind11::arg("stride"), pybind11::arg("na"), pybind11::arg("nc"), pybind11::arg("conf_thres") = 0.25,
        pybind11::arg("iou_thres") = 0.45, pybind11::arg("class_allow") = pybind11::none(),
        pybind11::arg("agnostic") = false, pybind11::arg("max_det") = 300, pybind11::arg("max_nms") = 30000,
        pybind11::arg("max_wh") = 7680.0, pybind11::arg("frame_map") = std::vector<double>(),
        pybind11::arg("det_out") = pybind11::none(), pybind11::arg("count_out") = pybind11::none());
  m.def("detect_workspace_bytes", [](int bs, int N) { return grpg_detect_workspace_bytes(bs, N); });
  // the detector's network: weight repack once, then the whole launch list in one call (detector.py)
  m.def("detector_pack_weights", &DetectorPackWeights);
  m.def("detector_run", &DetectorRun);
  m.def("detector_pack_weights_f16", &DetectorPackWeightsF16);
  m.def("detector_run_f16", &DetectorRunF16);
  // LPIPS: weight repack once, then the whole metric in one call; the leaves for the tests (lpips.py)
  m.def("lpips_pack_weights", &LpipsPackWeights);
  m.def("lpips_workspace_bytes", &LpipsWorkspaceBytes);
  m.def("lpips_workspace_map_offset", &LpipsWorkspaceMapOffset);
  m.def("lpips_forward", &LpipsForward);
  m.def("lpips_conv2d", &LpipsConv2d);
  m.def("lpips_max_pool", &LpipsMaxPool);
  m.def("lpips_distance", &LpipsDistance);
  // LPIPS as a loss: the forward that keeps its activations, the backward to x, and the backward's leaves
  m.def("lpips_train_workspace_bytes", &LpipsTrainWorkspaceBytes);
  m.def("lpips_train_activation_offset", &LpipsTrainActivationOffset);
  m.def("lpips_forward_train", &LpipsForwardTrain);
  m.def("lpips_bwd_pack_weights", &LpipsBwdPackWeights);
  m.def("lpips_backward", &LpipsBackward);
  m.def("lpips_conv2d_backward_data", &LpipsConv2dBackwardData);
  m.def("lpips_max_pool_backward", &LpipsMaxPoolBackward);
  m.def("lpips_distance_backward", &LpipsDistanceBackward);
  // the closed loop's tail: ranging alone, and the fused step (closed_loop.py)
  m.def("object_positions", &ObjectPositions);
  m.def("ego_loop_step", &EgoLoopStep);
  // tracklets -> actor poses (tracks.py): (rot [T,A,4], trans [T,A,3], active [T,A], chosen [T,A,4]) and the dense
  // (g_opt_trans [F,M,3], g_opt_rots [F,M,1])
  m.def("track_poses_forward", &TrackPosesForward, pybind11::arg("table"), pybind11::arg("timestamps"),
        pybind11::arg("ego"), pybind11::arg("opt_trans") = pybind11::none(), pybind11::arg("opt_rots") = pybind11::none(),
        pybind11::arg("val_stamps") = pybind11::none());
  m.def("track_poses_backward", &TrackPosesBackward, pybind11::arg("table"), pybind11::arg("timestamps"),
        pybind11::arg("ego"), pybind11::arg("opt_trans"), pybind11::arg("opt_rots"),
        pybind11::arg("val_stamps"), pybind11::arg("g_rot"), pybind11::arg("g_trans"));
  m.def("get_backward_timing", &BackwardTiming);   // (blend ms sum, preprocess ms sum, calls)
  m.def("set_stage_timing", [](int mode) { grpg_set_stage_timing(mode); });   // 0 off, 1 all, 2 render only
  m.def("stage_timing", &StageTiming);
  m.def("abi_version", []() { return grpg_abi_version(); });
  // 0 = speculative binning capacity + deferred num_rendered wait (default), 1 = exact (reference-like)
  m.def("set_binning_mode", [](int mode) {
    if (grpg_set_binning_mode(mode) != GRPG_OK) raise_abi_error("grpg_set_binning_mode", -1);
  });
  m.def("reset_capacity_hints", []() { grpg_reset_capacity_hints(); });
  // (P, width, height, instances, coarse pairs): exact capacities for the next forward of that shape
  m.def("set_capacity_hint", [](int P, int W, int H, unsigned R, unsigned Rc) {
    const int rc = grpg_set_capacity_hint(P, W, H, R, Rc);
    if (rc != GRPG_OK) raise_abi_error("grpg_set_capacity_hint", rc);
  });
  m.def("get_binning_algorithm", []() { return grpg_get_binning_algorithm(); });
  m.def("set_binning_algorithm", [](int alg) {
    if (grpg_set_binning_algorithm(alg) != GRPG_OK) raise_abi_error("grpg_set_binning_algorithm", -1);
  });
}

