// unet.hip -- the UNet of the anatomic-neck stage: the f32 / split-f16 runner, the 16-bit runners (the level-0 ping-pong kernels are
// unet16_pp.hip's), the work tickets of the persistent kernels, UNet turns between the contexts of a device, sh_unet_infer.
#include "sh_ctx.h"

#include "k_unet.h"
#include "k_unet_bf16.h"
#include "k_unet16_ldr.h"
#include "k_unet_x3.h"
#include "k_unet16_up.h"
#include "unet16_pp.h"

using namespace sh;

// ---- UNet forward (f32 MFMA path) ----------------------------------------------------------------------
static int conv_layer(sh_ctx* c, const char* lname, const sh_ctx::ULayer& L, const float* src0, const float* src1, int C0, int C1, float* dst,
                      int H, int W, int nimg, int relu, int fuse = 0, float* pooled = nullptr, const float* head_w = nullptr, const float* head_b = nullptr,
                      float* logits = nullptr, const float* image = nullptr, const float* w0 = nullptr, const float* b0 = nullptr) {
  if (H % UN_TH || W % UN_TW) return fail(c, SH_ERR_ARG, "unet: feature map is not a multiple of 16");
  const float* P = buf<float>(c, "params");
  const float* w = P + L.w_off; const float* b = P + L.b_off;
  const int tiles = (H / UN_TH) * (W / UN_TW);
  if (c->params.unet_dtype == SH_UNET_F32X && C0 % 32 == 0 && C1 % 32 == 0 && L.cout % 32 == 0) {
    // split-f16 operands on the 16-bit matrix pipe (k_unet_x3.h); weights split once per parameter block by unet_forward
    const u16* wh = buf<u16>(c, "params_x3h") + L.w_off;
    const u16* wl = buf<u16>(c, "params_x3l") + L.w_off;
    float* np_ = nullptr; const float* nf_ = nullptr;
    if (L.taps == 9 && fuse == (UF_FIRST | UF_POOL) && L.cout == 32 && C0 == 32 && C1 == 0) {      // enc0b with enc0a computed while its halo tile is staged
      LAUNCH(c, lname, (k_conv_mfma_x3<9, 2, UF_FIRST | UF_POOL, 0>), dim3(tiles, 1, nimg), dim3(UN_THREADS), src0, src1, C0, C1, wh, wl, b, dst, H, W, L.cout, relu, pooled, nf_, nf_, np_, image, w0, b0);
    }
    else if (L.taps == 9 && fuse == UF_HEAD && L.cout == 32) { LAUNCH(c, lname, (k_conv_mfma_x3<9, 2, UF_HEAD>), dim3(tiles, 1, nimg), dim3(UN_THREADS), src0, src1, C0, C1, wh, wl, b, dst, H, W, L.cout, relu, np_, head_w, head_b, logits, nf_, nf_, nf_); }
    else if (L.taps == 9 && fuse == UF_POOL && L.cout % 64 == 0) { LAUNCH(c, lname, (k_conv_mfma_x3<9, 4, UF_POOL>), dim3(tiles, L.cout / 64, nimg), dim3(UN_THREADS), src0, src1, C0, C1, wh, wl, b, dst, H, W, L.cout, relu, pooled, nf_, nf_, np_, nf_, nf_, nf_); }
    else if (L.taps == 9 && fuse == UF_POOL) { LAUNCH(c, lname, (k_conv_mfma_x3<9, 2, UF_POOL, 0>), dim3(tiles, L.cout / 32, nimg), dim3(UN_THREADS), src0, src1, C0, C1, wh, wl, b, dst, H, W, L.cout, relu, pooled, nf_, nf_, np_, nf_, nf_, nf_); }
    else if (fuse != 0) return fail(c, SH_ERR_ARG, "unet: unsupported fusion");
    else if (L.taps == 9 && L.cout % 64 == 0) { LAUNCH(c, lname, (k_conv_mfma_x3<9, 4>), dim3(tiles, L.cout / 64, nimg), dim3(UN_THREADS), src0, src1, C0, C1, wh, wl, b, dst, H, W, L.cout, relu, np_, nf_, nf_, np_, nf_, nf_, nf_); }
    else if (L.taps == 9) { LAUNCH(c, lname, (k_conv_mfma_x3<9, 2, 0, 0>), dim3(tiles, L.cout / 32, nimg), dim3(UN_THREADS), src0, src1, C0, C1, wh, wl, b, dst, H, W, L.cout, relu, np_, nf_, nf_, np_, nf_, nf_, nf_); }
    else if (C1 == 0 && W % 32 == 0 && H % 16 == 0 && (C0 == 64 || C0 == 128 || C0 == 256 || C0 == 512)) {
      // up-convolutions with the source pixels resident in registers (k_upconv_x3r)
      if (C0 == 64) { LAUNCH(c, lname, (k_upconv_x3r<2, 4>), dim3((W / 32) * (H / 16), nimg), dim3(UXR_THREADS), src0, wh, wl, b, dst, H, W, L.cout); }
      else if (C0 == 128) { LAUNCH(c, lname, (k_upconv_x3r<4, 4>), dim3((W / 32) * (H / 16), nimg), dim3(UXR_THREADS), src0, wh, wl, b, dst, H, W, L.cout); }
      else if (C0 == 256) { LAUNCH(c, lname, (k_upconv_x3r<8, 2>), dim3((W / 32) * (H / 8), nimg), dim3(UXR_THREADS), src0, wh, wl, b, dst, H, W, L.cout); }
      else { LAUNCH(c, lname, (k_upconv_x3r<16, 1>), dim3((W / 32) * (H / 4), nimg), dim3(UXR_THREADS), src0, wh, wl, b, dst, H, W, L.cout); }
    }
    else if (L.cout % 64 == 0) { LAUNCH(c, lname, (k_conv_mfma_x3<1, 4>), dim3(tiles, L.cout / 64, nimg * 4), dim3(UN_THREADS), src0, src1, C0, C1, wh, wl, b, dst, H, W, L.cout, 0, np_, nf_, nf_, np_, nf_, nf_, nf_); }
    else { LAUNCH(c, lname, (k_conv_mfma_x3<1, 2>), dim3(tiles, L.cout / 32, nimg * 4), dim3(UN_THREADS), src0, src1, C0, C1, wh, wl, b, dst, H, W, L.cout, 0, np_, nf_, nf_, np_, nf_, nf_, nf_); }
    return SH_OK;
  }
  if (L.taps == 9) {
    if (L.cout % 64 == 0) {
      LAUNCH(c, lname, (k_conv_mfma_f32<9, 4>), dim3(tiles, L.cout / 64, nimg), dim3(UN_THREADS), src0, src1, C0, C1, w, b, dst, H, W, L.cout, relu);
    } else {
      LAUNCH(c, lname, (k_conv_mfma_f32<9, 2>), dim3(tiles, L.cout / 32, nimg), dim3(UN_THREADS), src0, src1, C0, C1, w, b, dst, H, W, L.cout, relu);
    }
  } else {
    if (L.cout % 64 == 0) {
      LAUNCH(c, lname, (k_conv_mfma_f32<1, 4>), dim3(tiles, L.cout / 64, nimg * 4), dim3(UN_THREADS), src0, src1, C0, C1, w, b, dst, H, W, L.cout, 0);
    } else {
      LAUNCH(c, lname, (k_conv_mfma_f32<1, 2>), dim3(tiles, L.cout / 32, nimg * 4), dim3(UN_THREADS), src0, src1, C0, C1, w, b, dst, H, W, L.cout, 0);
    }
  }
  return SH_OK;
}

// ---- UNet turns ----------------------------------------------------------------------------------------
// Several contexts on one device overlap well when the launch-bound geometry kernels of one run beside the chip-filling
// UNet kernels of another -- and badly when two UNet passes share the CUs (each just takes twice as long).  Contexts
// that opted in (sh_set_unet_turns) therefore chain their UNet passes with events, in the order the host enqueued them.
static std::mutex g_turn_mu;
static hipEvent_t g_turn_last[64] = {};      // per device: recorded at the end of the most recently enqueued UNet pass
static sh_ctx* g_turn_owner[64] = {};

namespace sh {

int unet_turn_enter(sh_ctx* c) {
  if (!c->unet_turn || c->device < 0 || c->device >= 64) return SH_OK;
  std::lock_guard<std::mutex> lk(g_turn_mu);
  if (g_turn_last[c->device] && g_turn_owner[c->device] != c) HIPCHK(c, hipStreamWaitEvent(c->stream, g_turn_last[c->device], 0));
  return SH_OK;
}

int unet_turn_leave(sh_ctx* c) {
  if (!c->unet_turn || c->device < 0 || c->device >= 64) return SH_OK;
  std::lock_guard<std::mutex> lk(g_turn_mu);
  if (!c->unet_done_ev) HIPCHK(c, hipEventCreateWithFlags(&c->unet_done_ev, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->unet_done_ev, c->stream));
  g_turn_last[c->device] = c->unet_done_ev;
  g_turn_owner[c->device] = c;
  return SH_OK;
}

void unet_turn_forget(sh_ctx* c) {
  std::lock_guard<std::mutex> lk(g_turn_mu);
  if (c->device >= 0 && c->device < 64 && g_turn_owner[c->device] == c) { g_turn_last[c->device] = nullptr; g_turn_owner[c->device] = nullptr; }
}

}  // namespace sh

static int unet_forward(sh_ctx* c, const float* image, float* logits, int nimg, int H, int W) {
  const int D = c->unet_depth, base = c->unet_base;
  if ((H >> D) % 16 || (W >> D) % 16) return fail(c, SH_ERR_ARG, "unet: input size must be a multiple of 16 << depth");
  int rc;
  const size_t full = (size_t)nimg * H * W * base * 4;
  if ((rc = ensure(c, "unet.a", full, 4)) != SH_OK) return rc;
  if ((rc = ensure(c, "unet.b", full, 4)) != SH_OK) return rc;
  std::vector<float*> skip(D);
  for (int i = 0; i < D; ++i) {
    std::string nm = "unet.skip" + std::to_string(i);
    if ((rc = ensure(c, nm.c_str(), full >> i, 4)) != SH_OK) return rc;     // H*W/4^i * base*2^i
    skip[i] = buf<float>(c, nm.c_str());
  }
  float* A = buf<float>(c, "unet.a");
  float* Bq = buf<float>(c, "unet.b");
  const float* P = buf<float>(c, "params");
  if (c->params.unet_dtype == SH_UNET_F32X) {      // split the MFMA layers' weights into f16 high / low parts: one launch, once per parameter block
    if ((rc = ensure(c, "params_x3h", c->unet_floats * 2, 2)) != SH_OK) return rc;
    if ((rc = ensure(c, "params_x3l", c->unet_floats * 2, 2)) != SH_OK) return rc;
    if (!c->packed_x3) {
      std::vector<PackEntry> tab;
      long long total = 0;
      for (auto& kv : c->ulayers) {
        const sh_ctx::ULayer& l = kv.second;
        if (l.cin < 32 || l.cout < 32) continue;
        tab.push_back(PackEntry{total, (long long)l.w_off, l.taps, l.cin, l.cout, 0});
        total += (long long)l.taps * l.cin * l.cout;
        // range of the split: 64 w must be a finite f16 (|w| < 65504 / 64); beyond it the high part is an infinity and the layer's
        // outputs NaN, silently (include/shoulder_hip.h, SH_UNET_F32X)
        if (c->h_unet.size() >= l.w_off + (size_t)l.taps * l.cin * l.cout) {
          const float* wl = c->h_unet.data() + l.w_off;
          for (size_t i = 0, n = (size_t)l.taps * l.cin * l.cout; i < n; ++i)
            if (!(fabsf(wl[i]) < 65504.0f / X3_WSCALE)) {
              char m[200];
              snprintf(m, sizeof m, "SH_UNET_F32X: layer %s has a weight of magnitude %g; the split-f16 operands hold |w| < %g (use SH_UNET_F32 for this network)",
                       kv.first.c_str(), (double)fabsf(wl[i]), (double)(65504.0f / X3_WSCALE));
              return fail(c, SH_ERR_ARG, m);
            }
        }
      }
      if ((rc = ensure(c, "unet16.packtab", tab.size() * sizeof(PackEntry), 8)) != SH_OK) return rc;
      HIPCHK(c, hipMemcpyAsync(c->bufs["unet16.packtab"].p, tab.data(), tab.size() * sizeof(PackEntry), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));      // `tab` is a local
      c->packtab_ready = true;
      LAUNCH(c, "k_pack_w_x3", k_pack_w_x3, dim3(2048), dim3(256), P, buf<u16>(c, "params_x3h"), buf<u16>(c, "params_x3l"), (const PackEntry*)c->bufs["unet16.packtab"].p, (int)tab.size(), total);
      c->packed_x3 = true;
    }
  }
  auto L = [&](const std::string& n) -> const sh_ctx::ULayer& { return c->ulayers[n]; };
  int h = H, w = W;
  // SH_UNET_F32X: the 2x2 pools ride in the epilogue of the conv before them (k_unet_x3.h), and with 32 base channels the first
  // conv is computed inside enc0b's staging
  const bool x3 = c->params.unet_dtype == SH_UNET_F32X && base % 32 == 0;
  const bool x3_first = x3 && base == 32;
  if (!x3_first) {
    const sh_ctx::ULayer& l = L("enc0a");
    size_t npx = (size_t)nimg * h * w;
    LAUNCH(c, "unet.enc0a", k_conv_first, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 8192)), dim3(256), image, P + l.w_off, P + l.b_off, A, h, w, l.cout, nimg);
  }
  if (x3_first) {
    const sh_ctx::ULayer& l = L("enc0a");
    if ((rc = conv_layer(c, "unet.enc0b", L("enc0b"), A, nullptr, base, 0, skip[0], h, w, nimg, 1, UF_FIRST | UF_POOL, Bq, nullptr, nullptr, nullptr, image, P + l.w_off, P + l.b_off)) != SH_OK) return rc;
  } else if ((rc = conv_layer(c, "unet.enc0b", L("enc0b"), A, nullptr, base, 0, skip[0], h, w, nimg, 1, x3 ? UF_POOL : 0, Bq)) != SH_OK) return rc;
  if (x3) std::swap(A, Bq);      // (the pooled tensor is the next level's input, which the loop below reads from A)
  int ch = base;
  for (int i = 1; i <= D; ++i) {
    if (!x3) {
      size_t e = (size_t)nimg * (h / 2) * (w / 2) * (ch / 4);
      LAUNCH(c, "unet.pool", k_maxpool2, dim3((unsigned)std::min<size_t>((e + 255) / 256, 8192)), dim3(256), skip[i - 1], A, h, w, ch, nimg);
    }
    h /= 2; w /= 2;
    std::string na = i < D ? "enc" + std::to_string(i) + "a" : "bota", nb = i < D ? "enc" + std::to_string(i) + "b" : "botb";
    if ((rc = conv_layer(c, ("unet." + na).c_str(), L(na), A, nullptr, ch, 0, Bq, h, w, nimg, 1)) != SH_OK) return rc;
    ch *= 2;
    float* dst = i < D ? skip[i] : A;
    // (A was consumed by the conv above: with the fused pool it receives the next level's input)
    if ((rc = conv_layer(c, ("unet." + nb).c_str(), L(nb), Bq, nullptr, ch, 0, dst, h, w, nimg, 1, (x3 && i < D) ? UF_POOL : 0, A)) != SH_OK) return rc;
  }
  // decoder: x lives in A
  float* x = A; float* y = Bq;
  for (int i = D - 1; i >= 0; --i) {
    std::string nu = "up" + std::to_string(i), na = "dec" + std::to_string(i) + "a", nb = "dec" + std::to_string(i) + "b";
    if ((rc = conv_layer(c, ("unet." + nu).c_str(), L(nu), x, nullptr, ch, 0, y, h, w, nimg, 0)) != SH_OK) return rc;
    h *= 2; w *= 2; ch /= 2;
    if ((rc = conv_layer(c, ("unet." + na).c_str(), L(na), skip[i], y, ch, ch, x, h, w, nimg, 1)) != SH_OK) return rc;
    // (the head stays on k_head: its sequential f32 chain over the channels is the exact path's; fused into dec0b's epilogue the
    //  logits move by another ~1e-6 and one mask pixel of the 64-humerus bench batch flips)
    if ((rc = conv_layer(c, ("unet." + nb).c_str(), L(nb), x, nullptr, ch, 0, y, h, w, nimg, 1)) != SH_OK) return rc;
    std::swap(x, y);
  }
  {
    const sh_ctx::ULayer& l = L("head");
    size_t npx = (size_t)nimg * H * W;
    if (l.cin <= 32) { LAUNCH(c, "unet.head", k_head<32>, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 16384)), dim3(256), x, P + l.w_off, P + l.b_off, logits, l.cin, npx); }
    else { LAUNCH(c, "unet.head", k_head<64>, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 8192)), dim3(256), x, P + l.w_off, P + l.b_off, logits, l.cin, npx); }
  }
  return SH_OK;
}

// ---- UNet forward (16-bit MFMA paths: EK = 0 __bf16, 1 _Float16; tensors as raw u16) -----------------------------------------
#define SH_UNET_TICKETS 64
#define SH_UNET_TKTAB (1 << 18)
// Workgroups of a persistent UNet launch.  Each takes a whole CU (its LDS, all of its registers), so while one is resident no
// other kernel can start there: beside the UNet pass of one lane, every launch of the other lane's geometry chain (~40 per step)
// waited ~50 us for a workgroup to end, and the chain took 7-8 ms instead of 3.2.  Contexts that take turns on a device
// (sh_set_unet_turns: there IS another lane) therefore leave 32 CUs (4 per XCD) out of the grid; the work tickets spread the
// items over whatever grid there is.  Measured on the two-lane headline: 0 / 8 / 16 / 32 / 48 / 64 / 96 reserved -> 8.72 / 8.80 /
// 8.73 / 8.27 / 8.54 / 8.56 / 9.35 ms per step.
static int persistent_grid(sh_ctx* c) {
  constexpr int cu_reserve = 32;
  if (c->num_cus <= 0) { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) v = 0; c->num_cus = v > 0 ? v : 256; }
  return c->unet_turn ? std::max(8, c->num_cus - cu_reserve) : c->num_cus;
}

// work tickets of a persistent launch: the next free counter of this forward pass and the table of item bounds of runs of decreasing
// length for (items, workgroups, cout groups) -- every ticket a third of what would be a fair share of the remaining items, whole
// cout-group sets of a tile (its input tile comes from HBM once) -- built once per shape
static int unet_tickets(sh_ctx* c, int total, int nwg, int ngrp, unsigned** tk, const int** tk_tab, int* ntk) {
  const auto key = std::make_tuple(total, nwg, ngrp);
  auto it = c->tk_tabs.find(key);
  if (it == c->tk_tabs.end()) {
    std::vector<int> tab;
    int pos = 0;
    while (pos < total) {
      int sz = std::max(1, (int)std::ceil((total - pos) / (3.0 * (double)nwg)));
      if (sz >= ngrp) sz = sz / ngrp * ngrp;
      tab.push_back(pos);
      pos += std::min(sz, total - pos);
    }
    tab.push_back(total);
    if ((int)tab.size() > SH_UNET_TKTAB) return fail(c, SH_ERR_CAPACITY, "unet: ticket table larger than its buffer");
    if (c->tk_tab_used + (int)tab.size() > SH_UNET_TKTAB) {      // many different shapes (sh_unet_infer with varying n): start the cache over
      HIPCHK(c, hipStreamSynchronize(c->stream));                  // (launches that read the old tables are done)
      c->tk_tabs.clear();
      c->tk_tab_used = 0;
    }
    HIPCHK(c, hipMemcpyAsync(buf<int>(c, "unet16.tk_tab") + c->tk_tab_used, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // `tab` is a local
    it = c->tk_tabs.emplace(key, std::make_pair(c->tk_tab_used, (int)tab.size() - 1)).first;
    c->tk_tab_used += (int)tab.size();
  }
  if (c->ticket_next >= SH_UNET_TICKETS) return fail(c, SH_ERR_CAPACITY, "unet: out of work counters");
  *tk = buf<unsigned>(c, "unet16.tickets") + c->ticket_next++;
  *tk_tab = buf<int>(c, "unet16.tk_tab") + it->second.first;
  *ntk = it->second.second;
  return SH_OK;
}

// One layer of the 16-bit network.  3x3 convs with a multiple of 64 output channels on 32 x 16-tileable maps run on the persistent
// LDS-DMA kernel (k_unet16_ldr.h; UF_POOL: the 2x2 max pool written beside the output); 2x2 transposed convs on k_upconv16g /
// k_upconv16; everything else on the generic two-barrier kernel k_conv_mfma16 (k_unet_bf16.h), which is also the whole of the
// REFERENCE network (sh_ctx::unet_reference: layer by layer, nothing fused, no persistent kernel -- what the tests hold the
// production kernels against).
template <int EK>
static int conv_layer16(sh_ctx* c, const char* lname, const sh_ctx::ULayer& L, const u16* src0, const u16* src1, int C0, int C1,
                           u16* dst, int H, int W, int nimg, int relu, int fuse = 0, ConvFuse fz = ConvFuse{}) {
  if (H % UN_TH || W % UN_TW) return fail(c, SH_ERR_ARG, "unet: feature map is not a multiple of 16");
  const u16* w = buf<u16>(c, "params_bf16") + L.w_off;
  const float* b = buf<float>(c, "params") + L.b_off;
  const int tiles = (H / UN_TH) * (W / UN_TW);
  const dim3 blk(UN_THREADS);
  const bool ldr = !c->unet_reference && L.taps == 9 && L.cout % 64 == 0 && L.cout <= 512 && W % 32 == 0 && H % 16 == 0 && C0 % 32 == 0 && C1 % 32 == 0 &&
                   (fuse == 0 || (fuse == UF_POOL && relu));      // (its fused pool works on ReLU'd values)
  if (ldr) {
    int rc0;
    if ((rc0 = ensure(c, "unet16.zero", 256, 2)) != SH_OK) return rc0;
    if (!c->zero_page_ready) { HIPCHK(c, hipMemsetAsync(buf<char>(c, "unet16.zero"), 0, 256, c->stream)); c->zero_page_ready = true; }
    const int total = nimg * (W / 32) * (H / 16) * (L.cout / 64);
    const dim3 g((unsigned)std::min(total, persistent_grid(c)));
    unsigned* tk = nullptr; const int* tk_tab = nullptr; int ntk = 0;
    if ((rc0 = unet_tickets(c, total, (int)g.x, L.cout / 64, &tk, &tk_tab, &ntk)) != SH_OK) return rc0;
    const u16* zp = (const u16*)c->bufs["unet16.zero"].p;
    u16* pl = fuse == UF_POOL ? (u16*)fz.pooled : (u16*)nullptr;
    // weights resident in LDS: one cout group whose packed weights fit behind the two input buffers (32 -> 64 and 64 -> 64 layers)
    const bool wres = L.cout == 64 && ((C0 + C1) / 32) * 64 <= 128;
    if (fuse == UF_POOL && wres) { LAUNCH(c, lname, (k_conv3_ldr16<EK, UF_POOL, 1>), g, dim3(UD_THREADS), src0, src1, C0, C1, w, b, dst, H, W, L.cout, relu, nimg, zp, pl, tk, tk_tab, ntk); }
    else if (fuse == UF_POOL) { LAUNCH(c, lname, (k_conv3_ldr16<EK, UF_POOL, 0>), g, dim3(UD_THREADS), src0, src1, C0, C1, w, b, dst, H, W, L.cout, relu, nimg, zp, pl, tk, tk_tab, ntk); }
    else if (wres) { LAUNCH(c, lname, (k_conv3_ldr16<EK, 0, 1>), g, dim3(UD_THREADS), src0, src1, C0, C1, w, b, dst, H, W, L.cout, relu, nimg, zp, pl, tk, tk_tab, ntk); }
    else { LAUNCH(c, lname, (k_conv3_ldr16<EK, 0, 0>), g, dim3(UD_THREADS), src0, src1, C0, C1, w, b, dst, H, W, L.cout, relu, nimg, zp, pl, tk, tk_tab, ntk); }
  } else if (L.taps == 9 && L.cout % 64 == 0) {
    const dim3 g(tiles, L.cout / 64, nimg);
    if (fuse == 0) { LAUNCH(c, lname, (k_conv_mfma16<EK, 9, 4, 0>), g, blk, src0, src1, C0, C1, w, b, dst, H, W, L.cout, relu, fz); }
    else if (fuse == UF_POOL) { LAUNCH(c, lname, (k_conv_mfma16<EK, 9, 4, UF_POOL>), g, blk, src0, src1, C0, C1, w, b, dst, H, W, L.cout, relu, fz); }
    else return fail(c, SH_ERR_ARG, "unet: unsupported fusion");
  } else if (L.taps == 9) {
    const dim3 g(tiles, L.cout / 32, nimg);
    if (fuse == 0) { LAUNCH(c, lname, (k_conv_mfma16<EK, 9, 2, 0>), g, blk, src0, src1, C0, C1, w, b, dst, H, W, L.cout, relu, fz); }
    else return fail(c, SH_ERR_ARG, "unet: unsupported fusion");
  } else if (!c->unet_reference && L.cout % 32 == 0 && C1 == 0 && C0 % 32 == 0) {
    // 2x2 transposed conv (k_unet16_up.h): source pixels in registers, the weights of a 32-cout group by LDS-DMA, one barrier per
    // group (Cin = 512: per two phases); the staged form otherwise
    const bool upg = W % 32 == 0 && H % 16 == 0 && (C0 == 128 || C0 == 256 || C0 == 512) && L.cout <= 512;
    if (upg) {
      // items = (image, source tile of 32 x 4 MT pixels) on the grid of the persistent convolutions, handed out by work tickets; up3 has
      // about one item per CU: one workgroup per item
      const int mt = C0 == 128 ? 4 : 2, nitems = (W / 32) * (H / (4 * mt)) * nimg;
      const int grid = C0 == 512 ? nitems : std::min(nitems, persistent_grid(c));
      unsigned* tk = nullptr; const int* tk_tab = nullptr; int ntk = 0;
      if (C0 != 512) { const int trc = unet_tickets(c, nitems, grid, 1, &tk, &tk_tab, &ntk); if (trc != SH_OK) return trc; }
      if (C0 == 128) { LAUNCH(c, lname, (k_upconv16g<EK, 4, 4, 4, true>), dim3((unsigned)grid), dim3(UPR_THREADS), src0, w, b, dst, H, W, L.cout, nimg, tk, tk_tab, ntk); }
      else if (C0 == 256) { LAUNCH(c, lname, (k_upconv16g<EK, 8, 2, 4, true>), dim3((unsigned)grid), dim3(UPR_THREADS), src0, w, b, dst, H, W, L.cout, nimg, tk, tk_tab, ntk); }
      else { LAUNCH(c, lname, (k_upconv16g<EK, 16, 2, 2, false>), dim3((unsigned)grid), dim3(UPR_THREADS), src0, w, b, dst, H, W, L.cout, nimg, tk, tk_tab, ntk); }
    }
    else { LAUNCH(c, lname, (k_upconv16<EK>), dim3(tiles, L.cout / 32, nimg * 2), dim3(UPC_THREADS), src0, C0, w, b, dst, H, W, L.cout); }
  } else if (L.cout % 64 == 0) {
    LAUNCH(c, lname, (k_conv_mfma16<EK, 1, 4, 0>), dim3(tiles, L.cout / 64, nimg * 4), blk, src0, src1, C0, C1, w, b, dst, H, W, L.cout, 0, fz);
  } else {
    LAUNCH(c, lname, (k_conv_mfma16<EK, 1, 2, 0>), dim3(tiles, L.cout / 32, nimg * 4), blk, src0, src1, C0, C1, w, b, dst, H, W, L.cout, 0, fz);
  }
  return SH_OK;
}

// does the 16-bit forward run its fused level-0 kernels (k_unet16_pp.h)?  (run_window asks: k_enc0_pp can read the unscaled image)
namespace sh {
bool unet16_level0_fused(const sh_ctx* c, int H, int W) {
  return !c->unet_reference && c->unet_base == 32 && c->unet_depth >= 1 && W % 32 == 0 && H % 16 == 0 && (H >> c->unet_depth) % 16 == 0 && (W >> c->unet_depth) % 16 == 0;
}
}  // namespace sh

// Double-conv UNet, 16-bit.  With 32 base channels the full-resolution level runs as three fused ping-pong kernels (k_unet16_pp.h:
// image -> enc0a -> enc0b -> skip0 + pool; up0 + dec0a; dec0b + head) and every 2x2 max pool rides in the epilogue of the conv before
// it.  Other widths, maps that do not tile, and the reference network run layer by layer.
template <int EK>
static int unet_forward16(sh_ctx* c, const float* image, float* logits, int nimg, int H, int W) {
  const int D = c->unet_depth, base = c->unet_base;
  if ((H >> D) % 16 || (W >> D) % 16) return fail(c, SH_ERR_ARG, "unet: input size must be a multiple of 16 << depth");
  int rc;
  if ((rc = ensure(c, "params_bf16", c->unet_floats * 2, 2)) != SH_OK) return rc;
  const float* P = buf<float>(c, "params");
  u16* PW = buf<u16>(c, "params_bf16");
  if (c->packed_kind != EK) {     // pack the MFMA layers' weights for this element type: one launch for all layers, once per parameter block
    std::vector<PackEntry> tab;
    long long total = 0;
    for (auto& kv : c->ulayers) {
      const sh_ctx::ULayer& l = kv.second;
      if (l.cin < 32 || l.cout < 32) continue;
      tab.push_back(PackEntry{total, (long long)l.w_off, l.taps, l.cin, l.cout, 0});
      total += (long long)l.taps * l.cin * l.cout;
    }
    if ((rc = ensure(c, "unet16.packtab", tab.size() * sizeof(PackEntry), 8)) != SH_OK) return rc;
    if (!c->packtab_ready) {
      HIPCHK(c, hipMemcpyAsync(c->bufs["unet16.packtab"].p, tab.data(), tab.size() * sizeof(PackEntry), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));      // `tab` is a local
      c->packtab_ready = true;
    }
    LAUNCH(c, "k_pack_w_bf16", k_pack_w16_all<EK>, dim3(2048), dim3(256), P, PW, (const PackEntry*)c->bufs["unet16.packtab"].p, (int)tab.size(), total);
    c->packed_kind = EK;
  }
  if ((rc = ensure(c, "unet16.tickets", SH_UNET_TICKETS * 4, 4)) != SH_OK) return rc;
  if ((rc = ensure(c, "unet16.tk_tab", SH_UNET_TKTAB * 4, 4)) != SH_OK) return rc;
  FILL(c, {buf<unsigned>(c, "unet16.tickets"), (size_t)SH_UNET_TICKETS * 4, 0});
  c->ticket_next = 0;
  const bool fused = unet16_level0_fused(c, H, W);      // level 0 on the ping-pong kernels, pools in the conv epilogues
  const size_t full = (size_t)nimg * H * W * base * 2;
  if ((rc = ensure(c, "unet16.a", full, 2)) != SH_OK) return rc;
  if ((rc = ensure(c, "unet16.b", full, 2)) != SH_OK) return rc;
  std::vector<u16*> skip(D);
  for (int i = 0; i < D; ++i) {
    std::string nm = "unet16.skip" + std::to_string(i);
    if ((rc = ensure(c, nm.c_str(), full >> i, 2)) != SH_OK) return rc;
    skip[i] = buf<u16>(c, nm.c_str());
  }
  u16* A = buf<u16>(c, "unet16.a");
  u16* Bq = buf<u16>(c, "unet16.b");
  auto L = [&](const std::string& n) -> const sh_ctx::ULayer& { return c->ulayers[n]; };
  if ((rc = ensure(c, "unet16.zero", 256, 2)) != SH_OK) return rc;
  if (!c->zero_page_ready) { HIPCHK(c, hipMemsetAsync(buf<char>(c, "unet16.zero"), 0, 256, c->stream)); c->zero_page_ready = true; }
  const u16* zp = (const u16*)c->bufs["unet16.zero"].p;
  int h = H, w = W;
  if (fused) {
    // level-0 encoder (k_enc0_pp): image -> enc0a -> LDS -> enc0b -> skip0 + pooled
    const sh_ctx::ULayer& la = L("enc0a");
    const sh_ctx::ULayer& lb = L("enc0b");
    const int total = nimg * (w / 32) * (h / 16);
    const unsigned grid = (unsigned)std::min(total, persistent_grid(c));
    unsigned* tk = nullptr; const int* tk_tab = nullptr; int ntk = 0;
    if ((rc = unet_tickets(c, total, (int)grid, 1, &tk, &tk_tab, &ntk)) != SH_OK) return rc;
    LAUNCH_FN(c, "unet.enc0b", launch_enc0_pp(EK, grid, c->stream, image, P + la.w_off, P + la.b_off, PW + lb.w_off, P + lb.b_off, skip[0], A, h, w, nimg,
                                              c->unet_raw, c->unet_mm, tk, tk_tab, ntk));
  } else {
    const sh_ctx::ULayer& l = L("enc0a");
    size_t npx = (size_t)nimg * h * w;
    LAUNCH(c, "unet.enc0a", k_conv_first16<EK>, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 8192)), dim3(256), image, P + l.w_off, P + l.b_off, A, h, w, l.cout, nimg);
    if ((rc = conv_layer16<EK>(c, "unet.enc0b", L("enc0b"), A, nullptr, base, 0, skip[0], h, w, nimg, 1)) != SH_OK) return rc;
  }
  int ch = base;
  for (int i = 1; i <= D; ++i) {
    if (!fused) {
      size_t e = (size_t)nimg * (h / 2) * (w / 2) * (ch / 8);
      LAUNCH(c, "unet.pool", k_maxpool2_16<EK>, dim3((unsigned)std::min<size_t>((e + 255) / 256, 8192)), dim3(256), skip[i - 1], A, h, w, ch, nimg);
    }
    h /= 2; w /= 2;
    std::string na = i < D ? "enc" + std::to_string(i) + "a" : "bota", nb = i < D ? "enc" + std::to_string(i) + "b" : "botb";
    if ((rc = conv_layer16<EK>(c, ("unet." + na).c_str(), L(na), A, nullptr, ch, 0, Bq, h, w, nimg, 1)) != SH_OK) return rc;
    ch *= 2;
    u16* dst = i < D ? skip[i] : A;
    ConvFuse fz{};
    fz.pooled = A;      // (A was consumed by the conv above; the next level reads it)
    if ((rc = conv_layer16<EK>(c, ("unet." + nb).c_str(), L(nb), Bq, nullptr, ch, 0, dst, h, w, nimg, 1, (fused && i < D) ? UF_POOL : 0, fz)) != SH_OK) return rc;
  }
  u16* x = A; u16* y = Bq;
  for (int i = D - 1; i >= 0; --i) {
    std::string nu = "up" + std::to_string(i), na = "dec" + std::to_string(i) + "a", nb = "dec" + std::to_string(i) + "b";
    if (fused && i == 0) {
      // level 0: the up-convolution computed inside dec0a (k_dec0a_up_pp: x = low-resolution input, y = dec0a's output), then
      // dec0b with the 1x1 head in its epilogue (k_dec0b_head_pp: only the logits leave the kernel)
      h *= 2; w *= 2; ch /= 2;
      const sh_ctx::ULayer& lu = L(nu);
      const sh_ctx::ULayer& la = L(na);
      const sh_ctx::ULayer& lb = L(nb);
      const sh_ctx::ULayer& lh = L("head");
      {
        const int total = nimg * (w / 32) * (h / 8);
        const unsigned grid = (unsigned)std::min(total, persistent_grid(c));
        unsigned* tk = nullptr; const int* tk_tab = nullptr; int ntk = 0;
        if ((rc = unet_tickets(c, total, (int)grid, 1, &tk, &tk_tab, &ntk)) != SH_OK) return rc;
        LAUNCH_FN(c, "unet.dec0a", launch_dec0a_up_pp(EK, grid, c->stream, skip[0], x, PW + la.w_off, P + la.b_off, PW + lu.w_off, P + lu.b_off, y, h, w, nimg,
                                                      zp, tk, tk_tab, ntk));
      }
      {
        const int total = nimg * (w / 32) * (h / 16);
        const unsigned grid = (unsigned)std::min(total, persistent_grid(c));
        unsigned* tk = nullptr; const int* tk_tab = nullptr; int ntk = 0;
        if ((rc = unet_tickets(c, total, (int)grid, 1, &tk, &tk_tab, &ntk)) != SH_OK) return rc;
        LAUNCH_FN(c, "unet.dec0b", launch_dec0b_head_pp(EK, grid, c->stream, y, PW + lb.w_off, P + lb.b_off, P + lh.w_off, P + lh.b_off, logits, h, w, nimg,
                                                        zp, tk, tk_tab, ntk));
      }
      return SH_OK;
    }
    if ((rc = conv_layer16<EK>(c, ("unet." + nu).c_str(), L(nu), x, nullptr, ch, 0, y, h, w, nimg, 0)) != SH_OK) return rc;
    h *= 2; w *= 2; ch /= 2;
    if ((rc = conv_layer16<EK>(c, ("unet." + na).c_str(), L(na), skip[i], y, ch, ch, x, h, w, nimg, 1)) != SH_OK) return rc;
    if ((rc = conv_layer16<EK>(c, ("unet." + nb).c_str(), L(nb), x, nullptr, ch, 0, y, h, w, nimg, 1)) != SH_OK) return rc;
    std::swap(x, y);
  }
  {
    const sh_ctx::ULayer& l = L("head");
    size_t npx = (size_t)nimg * H * W;
    LAUNCH(c, "unet.head", k_head16<EK>, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 8192)), dim3(256), x, P + l.w_off, P + l.b_off, logits, l.cin, npx, (size_t)H * W);
  }
  return SH_OK;
}

namespace sh {
int unet_dispatch(sh_ctx* c, const float* image, float* logits, int nimg, int H, int W) {
  switch (c->params.unet_dtype) {
    case SH_UNET_BF16: return unet_forward16<0>(c, image, logits, nimg, H, W);
    case SH_UNET_F16: return unet_forward16<1>(c, image, logits, nimg, H, W);
    default: return unet_forward(c, image, logits, nimg, H, W);
  }
}
}  // namespace sh

extern "C" {

// The network alone (the `ort.InferenceSession.run` call of anatomic_neck.py:67-76): n images
// [n][H][W] float32 on the host -> logits [n][H][W] float32 on the host, in the precision sh_params.unet_dtype selects.
int sh_unet_infer(sh_ctx* c, const float* images, int n, int H, int W, float* logits) {
  if (!c || !images || !logits || n <= 0 || H <= 0 || W <= 0) return fail(c, SH_ERR_ARG, "sh_unet_infer: bad argument");
  if (c->ulayers.empty()) return fail(c, SH_ERR_STATE, "sh_unet_infer: no UNet weights loaded");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)n * H * W * 4;
  int rc;
  if ((rc = ensure(c, "infer.image", bytes, 4)) != SH_OK) return rc;
  if ((rc = ensure(c, "infer.logits", bytes, 4)) != SH_OK) return rc;
  WindowScope whole(c, 0, c->Bwin);      // named buffers below are whole-batch
  HIPCHK(c, hipMemcpyAsync(buf<float>(c, "infer.image"), images, bytes, hipMemcpyHostToDevice, c->stream));
  rc = unet_dispatch(c, buf<float>(c, "infer.image"), buf<float>(c, "infer.logits"), n, H, W);
  if (rc != SH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
  HIPCHK(c, hipMemcpyAsync(logits, buf<float>(c, "infer.logits"), bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

}  // extern "C"
