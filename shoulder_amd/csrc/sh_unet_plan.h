// sh_unet_plan.h -- what the UNet runner decides on the host before it launches anything: the layers of a network in the order of the
// parameter block (what sh_load_unet takes), the steps of one forward pass (which kernel with which template arguments, grid, block,
// tensors, fusions, work tickets), the run-length table of a ticketed launch, and the layer table of the weight-packing kernels.  No kernels, no HIP types: unet.hip includes it, and so does a plain g++
// (tests/hostcheck/unet_plan_check.cpp).  unet.hip holds the constants restated here against the kernel headers (static_assert).
#pragma once
#include "../../include/shoulder_hip.h"
#include "sh_common.h"      // (SH_UNET_MAXBASE)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

namespace sh {

struct UnetLayer { size_t w_off, b_off; int cin, cout, taps; };      // offsets in floats into the parameter block
typedef std::map<std::string, UnetLayer> UnetLayers;
struct UnetError { int code; std::string text; };      // code SH_OK: accepted

// The layers of the double-conv UNet in the order their parameters lie in the block (each layer's weights [taps][cin][cout], then its
// bias), with their offsets; *n_floats: the floats of the whole network.  The one statement of sh_load_unet's `packed` order.
struct UnetNamedLayer { std::string name; UnetLayer L; };
static inline std::vector<UnetNamedLayer> unet_layers_in_block_order(int base, int depth, size_t* n_floats) {
  std::vector<UnetNamedLayer> out;
  size_t o = 0;
  auto add = [&](const std::string& name, int taps, int cin, int cout) {
    const size_t nw = (size_t)taps * cin * cout;
    out.push_back({name, UnetLayer{o, o + nw, cin, cout, taps}});
    o += nw + cout;
  };
  auto ch = [base](int i) { return base << i; };
  for (int i = 0; i < depth; ++i) {
    add("enc" + std::to_string(i) + "a", 9, i ? ch(i - 1) : 1, ch(i));
    add("enc" + std::to_string(i) + "b", 9, ch(i), ch(i));
  }
  add("bota", 9, ch(depth - 1), ch(depth));
  add("botb", 9, ch(depth), ch(depth));
  for (int i = depth - 1; i >= 0; --i) {
    add("up" + std::to_string(i), 4, ch(i + 1), ch(i));
    add("dec" + std::to_string(i) + "a", 9, 2 * ch(i), ch(i));
    add("dec" + std::to_string(i) + "b", 9, ch(i), ch(i));
  }
  add("head", 1, ch(0), 1);
  *n_floats = o;
  return out;
}
// ... their names (the caller's arrays are <name>_w, <name>_b)
static inline std::vector<std::string> unet_layer_names(int depth) {
  size_t n;
  std::vector<std::string> names;
  for (const UnetNamedLayer& l : unet_layers_in_block_order(32, depth, &n)) names.push_back(l.name);
  return names;
}
// ... by name, for the networks the kernels are sized for: what sh_load_unet takes
#define SH_UNET_SHAPE_REFUSAL "sh_load_unet: bad argument (base must be a multiple of 32, at most 256; depth 1..6)"
static inline UnetError unet_layer_table(int base, int depth, UnetLayers* out, size_t* n_floats) {
  static_assert(SH_UNET_MAXBASE == 256, "SH_UNET_SHAPE_REFUSAL names the largest base");
  out->clear();
  *n_floats = 0;
  if (depth < 1 || depth > 6 || base < 32 || base % 32 != 0 || base > SH_UNET_MAXBASE) return {SH_ERR_ARG, SH_UNET_SHAPE_REFUSAL};
  for (const UnetNamedLayer& l : unet_layers_in_block_order(base, depth, n_floats)) (*out)[l.name] = l.L;
  return {SH_OK, {}};
}

// restated from the kernel headers: tile and block sizes, fusion flags (k_unet_bf16.h), the weight scale of the split-f16 operands
enum { PL_TILE = 16, PL_UN_THREADS = 256, PL_UD_THREADS = 512, PL_UPR_THREADS = 512, PL_UPC_THREADS = 256, PL_UXR_THREADS = 512 };
enum { PL_FIRST = 1, PL_HEAD = 2, PL_POOL = 4 };
constexpr float PL_X3_WSCALE = 64.0f;

// one value per kernel template; UnetStep::t holds the template arguments behind the element kind, in the template's order
enum UnetKernel {
  UK_CONV_FIRST, UK_MAXPOOL2, UK_HEAD /*<MAXC>*/, UK_CONV_F32 /*<TAPS, NT>*/, UK_CONV_X3 /*<TAPS, NT, FUSE, DB>*/, UK_UPCONV_X3R /*<NCH, MT>*/,
  UK_CONV_FIRST16, UK_MAXPOOL2_16, UK_HEAD16, UK_CONV16 /*<EK, TAPS, NT, FUSE>*/, UK_CONV3_LDR16 /*<EK, FUSE, WRES>*/,
  UK_UPCONV16G /*<EK, NCH, MT, PPB, PERSIST>*/, UK_UPCONV16 /*<EK>*/,
  UK_ENC0_PP /*<EK, RAW>: enc0a + enc0b + pool*/, UK_DEC0A_UP_PP /*<EK>: up0 + dec0a*/, UK_DEC0B_HEAD_PP /*<EK>: dec0b + head*/
};

// tensors of a pass: the two full-size buffers the layers alternate between, one skip tensor per level
enum { US_NONE = -1, US_IMAGE, US_A, US_B, US_LOGITS, US_SKIP /* + level */ };

struct UnetStep {
  std::string timer;                    // "unet.<layer>", "unet.pool"
  std::string layer, layer2;            // whose weights and bias it reads; layer2: the layer fused in (enc0a, up0, head), or empty
  UnetLayer L = {}, L2 = {};
  int kind = UK_CONV_FIRST, ek = -1;    // ek: 0 bf16, 1 f16, -1 the f32 kernels
  int t[4] = {0, 0, 0, 0};
  unsigned grid[3] = {1, 1, 1}, block = 0;      // block 0: the launcher's own (unet16_pp.hip)
  int C0 = 0, C1 = 0, H = 0, W = 0, cout = 0, relu = 0, fuse = 0;
  int src0 = US_NONE, src1 = US_NONE, dst = US_NONE, pool = US_NONE;      // pool: where a fused 2x2 max pool goes
  int tk_items = 0, tk_nwg = 0, tk_ngrp = 0;      // work tickets: (items, workgroups, cout groups); 0 items: none

  // the kernel in bench.py's spelling (sym_key): element kind by name, k_conv_mfma_x3 without its DB argument and with the pool bit
  // of FUSE only (enc0b with the first conv inside, <9, 2, UF_FIRST | UF_POOL, 0>, is bench's "<9,2,4>")
  std::string text() const {
    const char* e = ek == 1 ? "f16" : "bf16";
    char b[96];
    switch (kind) {
      case UK_CONV_FIRST: return "k_conv_first";
      case UK_MAXPOOL2: return "k_maxpool2";
      case UK_HEAD: snprintf(b, sizeof b, "k_head<%d>", t[0]); break;
      case UK_CONV_F32: snprintf(b, sizeof b, "k_conv_mfma_f32<%d,%d>", t[0], t[1]); break;
      case UK_CONV_X3: snprintf(b, sizeof b, "k_conv_mfma_x3<%d,%d,%d>", t[0], t[1], t[2] & ~PL_FIRST); break;
      case UK_UPCONV_X3R: snprintf(b, sizeof b, "k_upconv_x3r<%d,%d>", t[0], t[1]); break;
      case UK_CONV_FIRST16: snprintf(b, sizeof b, "k_conv_first16<%s>", e); break;
      case UK_MAXPOOL2_16: snprintf(b, sizeof b, "k_maxpool2_16<%s>", e); break;
      case UK_HEAD16: snprintf(b, sizeof b, "k_head16<%s>", e); break;
      case UK_CONV16: snprintf(b, sizeof b, "k_conv_mfma16<%s,%d,%d,%d>", e, t[0], t[1], t[2]); break;
      case UK_CONV3_LDR16: snprintf(b, sizeof b, "k_conv3_ldr16<%s,%d,%d>", e, t[0], t[1]); break;
      case UK_UPCONV16G: snprintf(b, sizeof b, "k_upconv16g<%s,%d,%d,%d,%s>", e, t[0], t[1], t[2], t[3] ? "true" : "false"); break;
      case UK_UPCONV16: snprintf(b, sizeof b, "k_upconv16<%s>", e); break;
      case UK_ENC0_PP: snprintf(b, sizeof b, "k_enc0_pp<%s,%s>", e, t[0] ? "true" : "false"); break;
      case UK_DEC0A_UP_PP: snprintf(b, sizeof b, "k_dec0a_up_pp<%s>", e); break;
      default: snprintf(b, sizeof b, "k_dec0b_head_pp<%s>", e); break;
    }
    return b;
  }
};

static inline bool unet_is16(int dtype) { return dtype == SH_UNET_BF16 || dtype == SH_UNET_F16; }

// does the pass run its full-resolution level on the three ping-pong kernels (k_unet16_pp.h)?  Then k_enc0_pp can read the unscaled
// image, which is why the stage runner asks too.
static inline bool plan_level0_fused(int dtype, bool reference, int base, int depth, int H, int W) {
  return unet_is16(dtype) && !reference && base == 32 && depth >= 1 && W % 32 == 0 && H % 16 == 0 && (H >> depth) % 16 == 0 && (W >> depth) % 16 == 0;
}

namespace plan_detail {

struct Conv { const char* name; int src0, src1, C0, C1, dst, relu, fuse, pool; };

struct Walk {
  const UnetLayers& layers;
  int dtype; bool reference; int nimg, pgrid;
  std::vector<UnetStep>* out;

  const UnetLayer* find(const std::string& n) const { auto it = layers.find(n); return it == layers.end() ? nullptr : &it->second; }

  UnetStep& add(const std::string& name, const UnetLayer& L, int kind, unsigned gx, unsigned gy, unsigned gz, unsigned block) {
    out->emplace_back();
    UnetStep& s = out->back();
    s.timer = "unet." + name; s.layer = name; s.L = L; s.kind = kind; s.ek = unet_is16(dtype) ? (dtype == SH_UNET_F16) : -1;
    s.grid[0] = gx; s.grid[1] = gy; s.grid[2] = gz; s.block = block; s.cout = L.cout;
    return s;
  }
  static void targs(UnetStep& s, int a, int b = 0, int c = 0, int d = 0) { s.t[0] = a; s.t[1] = b; s.t[2] = c; s.t[3] = d; }
  // a persistent launch: at most `pgrid` workgroups share `items`, handed out by work tickets over whole sets of `ngrp` cout groups
  void persistent(UnetStep& s, int items, int ngrp) const { s.grid[0] = (unsigned)std::min(items, pgrid); s.tk_items = items; s.tk_nwg = (int)s.grid[0]; s.tk_ngrp = ngrp; }
  // grid of the element-wise kernels (first conv, pool, head): 256 elements per workgroup, capped
  static unsigned flat_grid(size_t n, size_t cap) { return (unsigned)std::min<size_t>((n + 255) / 256, cap); }

  // One convolution layer: which kernel runs it.
  //   f32:   k_conv_mfma_f32.
  //   f32x:  split-f16 operands on the 16-bit matrix pipe (k_unet_x3.h); 2x2 transposed convs of 64 / 128 / 256 / 512 channels on 32 x 16
  //          tileable maps with the source pixels resident in registers (k_upconv_x3r).
  //   16-bit: 3x3 convs with a multiple of 64 output channels on 32 x 16-tileable maps on the persistent LDS-DMA kernel (k_unet16_ldr.h;
  //          UF_POOL: the 2x2 max pool written beside the output, on ReLU'd values); 2x2 transposed convs on k_upconv16g / k_upconv16;
  //          everything else on the generic two-barrier kernel k_conv_mfma16, which is also the whole of the REFERENCE network (layer by
  //          layer, nothing fused, no persistent kernel -- what the tests hold the production kernels against).
  UnetError conv(const Conv& q, int H, int W) {
    const UnetLayer* lp = find(q.name);
    if (!lp) return {SH_ERR_STATE, std::string("unet: no layer named ") + q.name};
    const UnetLayer& L = *lp;
    if (H % PL_TILE || W % PL_TILE) return {SH_ERR_ARG, "unet: feature map is not a multiple of 16"};
    const int tiles = (H / PL_TILE) * (W / PL_TILE), C0 = q.C0, C1 = q.C1, fuse = q.fuse, n64 = L.cout / 64, n32 = L.cout / 32;
    const bool c64 = L.cout % 64 == 0, tile32 = W % 32 == 0 && H % 16 == 0;
    const UnetError unsupported = {SH_ERR_ARG, "unet: unsupported fusion"};
    UnetStep* s = nullptr;
    int relu = q.relu;
    if (unet_is16(dtype)) {
      const bool ldr = !reference && L.taps == 9 && c64 && L.cout <= 512 && tile32 && C0 % 32 == 0 && C1 % 32 == 0 && (fuse == 0 || (fuse == PL_POOL && q.relu));
      if (ldr) {
        // weights resident in LDS: one cout group whose packed weights fit behind the two input buffers (32 -> 64 and 64 -> 64 layers)
        const bool wres = L.cout == 64 && ((C0 + C1) / 32) * 64 <= 128;
        s = &add(q.name, L, UK_CONV3_LDR16, 1, 1, 1, PL_UD_THREADS);
        targs(*s, fuse, wres);
        persistent(*s, nimg * (W / 32) * (H / 16) * n64, n64);
      } else if (L.taps == 9 && c64) {
        if (fuse != 0 && fuse != PL_POOL) return unsupported;
        s = &add(q.name, L, UK_CONV16, tiles, n64, nimg, PL_UN_THREADS);
        targs(*s, 9, 4, fuse);
      } else if (L.taps == 9) {
        if (fuse != 0) return unsupported;
        s = &add(q.name, L, UK_CONV16, tiles, n32, nimg, PL_UN_THREADS);
        targs(*s, 9, 2, 0);
      } else if (!reference && L.cout % 32 == 0 && C1 == 0 && C0 % 32 == 0) {
        // 2x2 transposed conv (k_unet16_up.h): source pixels in registers, the weights of a 32-cout group by LDS-DMA, one barrier per
        // group (Cin = 512: per two phases); the staged form otherwise
        if (tile32 && (C0 == 128 || C0 == 256 || C0 == 512) && L.cout <= 512) {
          // items = (image, source tile of 32 x 4 MT pixels) on the grid of the persistent convolutions, handed out by work tickets; up3
          // has about one item per CU: one workgroup per item
          const int mt = C0 == 128 ? 4 : 2, nitems = (W / 32) * (H / (4 * mt)) * nimg;
          s = &add(q.name, L, UK_UPCONV16G, nitems, 1, 1, PL_UPR_THREADS);
          targs(*s, C0 / 32, mt, C0 == 512 ? 2 : 4, C0 != 512);
          if (C0 != 512) persistent(*s, nitems, 1);
        } else {
          s = &add(q.name, L, UK_UPCONV16, tiles, n32, nimg * 2, PL_UPC_THREADS);
        }
      } else {
        s = &add(q.name, L, UK_CONV16, tiles, c64 ? n64 : n32, nimg * 4, PL_UN_THREADS);
        targs(*s, 1, c64 ? 4 : 2, 0);
        relu = 0;
      }
    } else if (dtype == SH_UNET_F32X && C0 % 32 == 0 && C1 % 32 == 0 && L.cout % 32 == 0) {
      if (L.taps == 9) {
        // DB (the double-buffered form) is the template's default except where NT = 2 runs without a head
        if (fuse == (PL_FIRST | PL_POOL) && L.cout == 32 && C0 == 32 && C1 == 0) { s = &add(q.name, L, UK_CONV_X3, tiles, 1, nimg, PL_UN_THREADS); targs(*s, 9, 2, fuse, 0); }
        else if (fuse == PL_HEAD && L.cout == 32) { s = &add(q.name, L, UK_CONV_X3, tiles, 1, nimg, PL_UN_THREADS); targs(*s, 9, 2, fuse, 1); }
        else if (fuse != 0 && fuse != PL_POOL) return unsupported;
        else if (c64) { s = &add(q.name, L, UK_CONV_X3, tiles, n64, nimg, PL_UN_THREADS); targs(*s, 9, 4, fuse, 1); }
        else { s = &add(q.name, L, UK_CONV_X3, tiles, n32, nimg, PL_UN_THREADS); targs(*s, 9, 2, fuse, 0); }
      } else if (fuse != 0) {
        return unsupported;
      } else if (C1 == 0 && tile32 && (C0 == 64 || C0 == 128 || C0 == 256 || C0 == 512)) {
        const int mt = C0 <= 128 ? 4 : C0 == 256 ? 2 : 1;
        s = &add(q.name, L, UK_UPCONV_X3R, (W / 32) * (H / (4 * mt)), nimg, 1, PL_UXR_THREADS);
        targs(*s, C0 / 32, mt);
      } else {
        s = &add(q.name, L, UK_CONV_X3, tiles, c64 ? n64 : n32, nimg * 4, PL_UN_THREADS);
        targs(*s, 1, c64 ? 4 : 2, 0, 1);
        relu = 0;
      }
    } else {
      const bool nine = L.taps == 9;
      s = &add(q.name, L, UK_CONV_F32, tiles, c64 ? n64 : n32, nine ? nimg : nimg * 4, PL_UN_THREADS);
      targs(*s, nine ? 9 : 1, c64 ? 4 : 2);
      if (!nine) relu = 0;
    }
    s->C0 = C0; s->C1 = C1; s->H = H; s->W = W; s->relu = relu; s->fuse = fuse;
    if (fuse & (PL_FIRST | PL_HEAD)) {      // the layer computed inside this one
      s->layer2 = (fuse & PL_FIRST) ? "enc0a" : "head";
      if (!(lp = find(s->layer2))) return {SH_ERR_STATE, "unet: no layer named " + s->layer2};
      s->L2 = *lp;
    }
    s->src0 = q.src0; s->src1 = q.src1; s->dst = q.dst; s->pool = (fuse & PL_POOL) ? q.pool : US_NONE;
    return {SH_OK, {}};
  }
};

}  // namespace plan_detail

// The steps of one forward pass of the double-conv UNet (enc0a, enc0b, per level pool + two convs down to bota / botb, per level
// up + two convs, the head), in launch order.  `pgrid`: workgroups of a persistent launch; `raw`: the caller has the unscaled image.
//   f32:    every layer and every pool a launch of its own.
//   f32x:   the 2x2 pools ride in the epilogue of the conv before them, and with 32 base channels the first conv is computed inside
//           enc0b's staging.  The head stays on k_head: its sequential f32 chain over the channels is the exact path's; fused into
//           dec0b's epilogue the logits move by another ~1e-6 and one mask pixel of the 64-humerus bench batch flips.
//   16-bit: with 32 base channels on maps that tile, the full-resolution level runs as three fused ping-pong kernels (k_unet16_pp.h:
//           image -> enc0a -> enc0b -> skip0 + pool; up0 + dec0a; dec0b + head) and every pool rides in the conv before it.  Other
//           widths, maps that do not tile, and the reference network run layer by layer like f32.
static inline UnetError unet_plan(const UnetLayers& layers, int base, int depth, int dtype, bool reference, int H, int W, int nimg, int pgrid, bool raw,
                                  std::vector<UnetStep>* out) {
  using namespace plan_detail;
  const int D = depth;
  if ((H >> D) % 16 || (W >> D) % 16) return {SH_ERR_ARG, "unet: input size must be a multiple of 16 << depth"};
  out->clear();
  out->reserve(6 * D + 8);
  Walk wk{layers, dtype, reference, nimg, pgrid, out};
  const bool b16 = unet_is16(dtype);
  const bool x3 = dtype == SH_UNET_F32X && base % 32 == 0, x3_first = x3 && base == 32;
  const bool fused = plan_level0_fused(dtype, reference, base, depth, H, W);
  const bool pools_fused = x3 || fused;
  auto L = [&](const std::string& n, const UnetLayer** l) -> UnetError {
    *l = wk.find(n);
    return *l ? UnetError{SH_OK, {}} : UnetError{SH_ERR_STATE, "unet: no layer named " + n};
  };
  UnetError e;
  const UnetLayer *la = nullptr, *lb = nullptr, *lu = nullptr, *lh = nullptr;
  if ((e = L("enc0a", &la)).code || (e = L("enc0b", &lb)).code || (e = L("head", &lh)).code) return e;
  int A = US_A, B = US_B, h = H, w = W, ch = base;
  if (fused) {
    UnetStep& s = wk.add("enc0b", *lb, UK_ENC0_PP, 1, 1, 1, 0);
    s.layer2 = "enc0a"; s.L2 = *la; Walk::targs(s, raw);
    wk.persistent(s, nimg * (w / 32) * (h / 16), 1);
    s.C0 = 1; s.H = h; s.W = w; s.relu = 1; s.fuse = PL_FIRST | PL_POOL; s.src0 = US_IMAGE; s.dst = US_SKIP; s.pool = A;
  } else {
    if (!x3_first) {
      UnetStep& s = wk.add("enc0a", *la, b16 ? UK_CONV_FIRST16 : UK_CONV_FIRST, Walk::flat_grid((size_t)nimg * h * w, 8192), 1, 1, 256);
      s.C0 = 1; s.H = h; s.W = w; s.relu = 1; s.src0 = US_IMAGE; s.dst = A;
    }
    if ((e = wk.conv({"enc0b", A, US_NONE, base, 0, US_SKIP, 1, x3_first ? PL_FIRST | PL_POOL : x3 ? PL_POOL : 0, B}, h, w)).code) return e;
    if (x3) std::swap(A, B);      // (the pooled tensor is the next level's input, which the loop below reads from A)
  }
  for (int i = 1; i <= D; ++i) {
    if (!pools_fused) {
      const size_t n = (size_t)nimg * (h / 2) * (w / 2) * (ch / (b16 ? 8 : 4));
      UnetStep& s = wk.add("pool", UnetLayer{}, b16 ? UK_MAXPOOL2_16 : UK_MAXPOOL2, Walk::flat_grid(n, 8192), 1, 1, 256);
      s.layer.clear(); s.C0 = ch; s.cout = ch; s.H = h; s.W = w; s.src0 = US_SKIP + i - 1; s.dst = A;
    }
    h /= 2; w /= 2;
    const std::string na = i < D ? "enc" + std::to_string(i) + "a" : "bota", nb = i < D ? "enc" + std::to_string(i) + "b" : "botb";
    if ((e = wk.conv({na.c_str(), A, US_NONE, ch, 0, B, 1, 0, US_NONE}, h, w)).code) return e;
    ch *= 2;
    // (A was consumed by the conv above: with the fused pool it receives the next level's input)
    if ((e = wk.conv({nb.c_str(), B, US_NONE, ch, 0, i < D ? US_SKIP + i : A, 1, (pools_fused && i < D) ? PL_POOL : 0, A}, h, w)).code) return e;
  }
  int x = A, y = B;      // decoder: x lives in A
  for (int i = D - 1; i >= 0; --i) {
    const std::string nu = "up" + std::to_string(i), na = "dec" + std::to_string(i) + "a", nb = "dec" + std::to_string(i) + "b";
    if (fused && i == 0) {
      // level 0: the up-convolution computed inside dec0a (k_dec0a_up_pp: x = low-resolution input, y = dec0a's output, 32 x 8 tiles),
      // then dec0b with the 1x1 head in its epilogue (k_dec0b_head_pp: only the logits leave the kernel)
      h *= 2; w *= 2; ch /= 2;
      if ((e = L(nu, &lu)).code || (e = L(na, &la)).code || (e = L(nb, &lb)).code) return e;
      UnetStep& a = wk.add(na, *la, UK_DEC0A_UP_PP, 1, 1, 1, 0);
      a.layer2 = nu; a.L2 = *lu;
      wk.persistent(a, nimg * (w / 32) * (h / 8), 1);
      a.C0 = ch; a.C1 = ch; a.H = h; a.W = w; a.relu = 1; a.src0 = US_SKIP; a.src1 = x; a.dst = y;
      UnetStep& b = wk.add(nb, *lb, UK_DEC0B_HEAD_PP, 1, 1, 1, 0);
      b.layer2 = "head"; b.L2 = *lh;
      wk.persistent(b, nimg * (w / 32) * (h / 16), 1);
      b.C0 = ch; b.H = h; b.W = w; b.relu = 1; b.fuse = PL_HEAD; b.src0 = y; b.dst = US_LOGITS;
      return {SH_OK, {}};
    }
    if ((e = wk.conv({nu.c_str(), x, US_NONE, ch, 0, y, 0, 0, US_NONE}, h, w)).code) return e;
    h *= 2; w *= 2; ch /= 2;
    if ((e = wk.conv({na.c_str(), US_SKIP + i, y, ch, ch, x, 1, 0, US_NONE}, h, w)).code) return e;
    if ((e = wk.conv({nb.c_str(), x, US_NONE, ch, 0, y, 1, 0, US_NONE}, h, w)).code) return e;
    std::swap(x, y);
  }
  const size_t npx = (size_t)nimg * H * W;
  const bool small = !b16 && lh->cin <= 32;
  UnetStep& s = wk.add("head", *lh, b16 ? UK_HEAD16 : UK_HEAD, Walk::flat_grid(npx, small ? 16384 : 8192), 1, 1, 256);
  if (!b16) Walk::targs(s, small ? 32 : 64);
  s.C0 = lh->cin; s.H = H; s.W = W; s.src0 = x; s.dst = US_LOGITS;
  return {SH_OK, {}};
}

// Item bounds of the work tickets of a persistent launch, in runs of decreasing length: every ticket a third of what would be a fair
// share of the remaining items, in whole cout-group sets of a tile (its input tile comes from HBM once).  n tickets: n + 1 bounds.
static inline std::vector<int> ticket_table(int total, int nwg, int ngrp) {
  std::vector<int> tab;
  int pos = 0;
  while (pos < total) {
    int sz = std::max(1, (int)std::ceil((total - pos) / (3.0 * (double)nwg)));
    if (sz >= ngrp) sz = sz / ngrp * ngrp;
    tab.push_back(pos);
    pos += std::min(sz, total - pos);
  }
  tab.push_back(total);
  return tab;
}

// The layers the weight-packing kernels pack (the MFMA layers: at least 32 channels in and out), in the layout of PackEntry
// (k_unet_bf16.h), and the packed elements in all.  `host_w` (the host copy of the parameter block, `host_n` floats; null: no check):
// the range of the split-f16 operands -- 64 w must be a finite f16 (|w| < 65504 / 64); beyond it the high part is an infinity and the
// layer's outputs NaN, silently (include/shoulder_hip.h, SH_UNET_F32X).
struct PackRow { long long first; long long w_off; int T, Cin, Cout, pad; };
static inline UnetError pack_table(const UnetLayers& layers, std::vector<PackRow>* tab, long long* total, const float* host_w = nullptr, size_t host_n = 0) {
  tab->clear();
  *total = 0;
  for (auto& kv : layers) {
    const UnetLayer& l = kv.second;
    if (l.cin < 32 || l.cout < 32) continue;
    const size_t n = (size_t)l.taps * l.cin * l.cout;
    tab->push_back(PackRow{*total, (long long)l.w_off, l.taps, l.cin, l.cout, 0});
    *total += (long long)n;
    if (!host_w || host_n < l.w_off + n) continue;
    for (size_t i = 0; i < n; ++i)
      if (!(std::fabs(host_w[l.w_off + i]) < 65504.0f / PL_X3_WSCALE)) {
        char m[200];
        snprintf(m, sizeof m, "SH_UNET_F32X: layer %s has a weight of magnitude %g; the split-f16 operands hold |w| < %g (use SH_UNET_F32 for this network)",
                 kv.first.c_str(), (double)std::fabs(host_w[l.w_off + i]), (double)(65504.0f / PL_X3_WSCALE));
        return {SH_ERR_ARG, m};
      }
  }
  return {SH_OK, {}};
}

}  // namespace sh
