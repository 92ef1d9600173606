// unet.hip -- the UNet of the anatomic-neck stage: one runner for the f32, split-f16 and 16-bit forms of the network (the level-0
// ping-pong kernels are unet16_pp.hip's).  sh_unet_plan.h decides the steps of a pass; here are the buffers, the launch of a step, the
// work tickets of the persistent kernels, weight packing, UNet turns between the contexts of a device, sh_unet_infer.
#include "sh_ctx.h"

#include "k_unet.h"
#include "k_unet_bf16.h"
#include "k_unet16_ldr.h"
#include "k_unet_x3.h"
#include "k_unet16_up.h"
#include "unet16_pp.h"

using namespace sh;

// what sh_unet_plan.h restates of the kernel headers
static_assert(PL_TILE == UN_TH && PL_TILE == UN_TW && PL_UN_THREADS == UN_THREADS && PL_UD_THREADS == UD_THREADS && PL_UPR_THREADS == UPR_THREADS &&
              PL_UPC_THREADS == UPC_THREADS && PL_UXR_THREADS == UXR_THREADS, "sh_unet_plan.h: tile / block sizes");
static_assert(PL_FIRST == UF_FIRST && PL_HEAD == UF_HEAD && PL_POOL == UF_POOL && PL_X3_WSCALE == X3_WSCALE, "sh_unet_plan.h: fusion flags, weight scale");
static_assert(sizeof(PackRow) == sizeof(PackEntry) && offsetof(PackRow, first) == offsetof(PackEntry, first) && offsetof(PackRow, w_off) == offsetof(PackEntry, w_off) &&
              offsetof(PackRow, T) == offsetof(PackEntry, T) && offsetof(PackRow, Cin) == offsetof(PackEntry, Cin) && offsetof(PackRow, Cout) == offsetof(PackEntry, Cout),
              "sh_unet_plan.h: PackRow is PackEntry");

// ---- UNet turns ----------------------------------------------------------------------------------------
// Several contexts on one device overlap well when the launch-bound geometry kernels of one run beside the chip-filling
// UNet kernels of another -- and badly when two UNet passes share the CUs (each just takes twice as long).  Contexts
// that opted in (sh_set_unet_turns) therefore chain their UNet passes with events, in the order the host enqueued them.
static std::mutex g_turn_mu;
static hipEvent_t g_turn_last[64] = {};      // per device: recorded at the end of the most recently enqueued UNet pass
static sh_ctx* g_turn_owner[64] = {};

namespace sh {

int unet_turn_enter(sh_ctx* c) {
  if (!c->unet.turn || c->device < 0 || c->device >= 64) return SH_OK;
  std::lock_guard<std::mutex> lk(g_turn_mu);
  if (g_turn_last[c->device] && g_turn_owner[c->device] != c) HIPCHK(c, hipStreamWaitEvent(c->stream, g_turn_last[c->device], 0));
  return SH_OK;
}

int unet_turn_leave(sh_ctx* c) {
  if (!c->unet.turn || c->device < 0 || c->device >= 64) return SH_OK;
  std::lock_guard<std::mutex> lk(g_turn_mu);
  if (!c->unet.done_ev) HIPCHK(c, hipEventCreateWithFlags(&c->unet.done_ev, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->unet.done_ev, c->stream));
  g_turn_last[c->device] = c->unet.done_ev;
  g_turn_owner[c->device] = c;
  return SH_OK;
}

void unet_turn_forget(sh_ctx* c) {
  std::lock_guard<std::mutex> lk(g_turn_mu);
  if (c->device >= 0 && c->device < 64 && g_turn_owner[c->device] == c) { g_turn_last[c->device] = nullptr; g_turn_owner[c->device] = nullptr; }
}

}  // namespace sh

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
  if (c->unet.num_cus <= 0) { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) v = 0; c->unet.num_cus = v > 0 ? v : 256; }
  return c->unet.turn ? std::max(8, c->unet.num_cus - cu_reserve) : c->unet.num_cus;
}

// The buffers of a pass, resolved once (none of them is windowed).  act: the tensors by slot (US_IMAGE, US_A, US_B, US_LOGITS,
// US_SKIP + level): float in the f32 forms, u16 in the 16-bit ones.
struct UnetView {
  UnetIO io;
  int nimg;
  const float* P;                      // "params"
  u16 *PW, *wh, *wl;                   // "params_bf16" | "params_x3h", "params_x3l"
  const u16* zero;                     // "unet16.zero"
  unsigned* tickets; int* tk_tab;      // "unet16.tickets", "unet16.tk_tab"
  void* act[US_SKIP + 6];              // (sh_load_unet: depth <= 6)
  template <typename T> T* at(int slot) const { return slot < 0 ? nullptr : (T*)act[slot]; }
};

static int unet_view(sh_ctx* c, const UnetIO& io, int nimg, int H, int W, UnetView* v) {
  const int dtype = c->params.unet_dtype, es = unet_is16(dtype) ? 2 : 4;
  const std::string pre = unet_is16(dtype) ? "unet16." : "unet.";
  const ParamShape& ps = c->pstate.shape();
  const size_t full = (size_t)nimg * H * W * ps.base * es;
  *v = UnetView{};
  v->io = io; v->nimg = nimg; v->P = buf<float>(c, "params");
  v->act[US_IMAGE] = (void*)io.image; v->act[US_LOGITS] = io.logits;
  int rc;
  if ((rc = ensure(c, (pre + "a").c_str(), full, es, &v->act[US_A])) != SH_OK) return rc;
  if ((rc = ensure(c, (pre + "b").c_str(), full, es, &v->act[US_B])) != SH_OK) return rc;
  for (int i = 0; i < ps.depth; ++i)      // H*W/4^i * base*2^i
    if ((rc = ensure(c, (pre + "skip" + std::to_string(i)).c_str(), full >> i, es, &v->act[US_SKIP + i])) != SH_OK) return rc;
  if (dtype == SH_UNET_F32X) {
    if ((rc = ensure(c, "params_x3h", ps.unet_floats * 2, 2, (void**)&v->wh)) != SH_OK) return rc;
    if ((rc = ensure(c, "params_x3l", ps.unet_floats * 2, 2, (void**)&v->wl)) != SH_OK) return rc;
  } else if (unet_is16(dtype)) {
    if ((rc = ensure(c, "params_bf16", ps.unet_floats * 2, 2, (void**)&v->PW)) != SH_OK) return rc;
    if ((rc = ensure(c, "unet16.tickets", SH_UNET_TICKETS * 4, 4, (void**)&v->tickets)) != SH_OK) return rc;
    if ((rc = ensure(c, "unet16.tk_tab", SH_UNET_TKTAB * 4, 4, (void**)&v->tk_tab)) != SH_OK) return rc;
    if ((rc = ensure(c, "unet16.zero", 256, 2, (void**)&v->zero)) != SH_OK) return rc;
  }
  return SH_OK;
}

// The MFMA layers' weights in the form the kernels read -- 16-bit (kind 0 bf16, 1 f16) or split into f16 high / low parts (kind -1):
// one launch for all layers, once per parameter block; the layer table goes up once per loaded network.
static int pack_weights(sh_ctx* c, const UnetView& v, int kind) {
  ParamState& ps = c->pstate;
  if (!(kind < 0 ? ps.need_pack_x3() : ps.need_pack16(kind))) return SH_OK;
  std::vector<PackRow> tab;
  long long total = 0;
  const UnetError e = pack_table(c->ulayers, &tab, &total, kind < 0 ? c->mirror.unet.data() : nullptr, c->mirror.unet.size());
  if (e.code != SH_OK) return fail(c, e.code, e.text);
  int rc;
  PackEntry* dtab = nullptr;
  if ((rc = ensure(c, "unet16.packtab", tab.size() * sizeof(PackRow), 8, (void**)&dtab)) != SH_OK) return rc;
  if (ps.need_packtab()) {
    HIPCHK(c, hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(PackRow), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // `tab` is a local
    ps.packtab_uploaded();
  }
  if (kind < 0) {
    LAUNCH(c, "k_pack_w_x3", k_pack_w_x3, dim3(2048), dim3(256), v.P, v.wh, v.wl, (const PackEntry*)dtab, (int)tab.size(), total);
    ps.packed_x3();
  } else {
    LAUNCH(c, "k_pack_w_bf16", (kind ? k_pack_w16_all<1> : k_pack_w16_all<0>), dim3(2048), dim3(256), v.P, v.PW, (const PackEntry*)dtab, (int)tab.size(), total);
    ps.packed16(kind);
  }
  return SH_OK;
}

// the page of zeros the LDS-DMA kernels read for pixels outside the image
static int zero_page(sh_ctx* c, const UnetView& v) {
  if (c->unet.zero_page_ready) return SH_OK;
  HIPCHK(c, hipMemsetAsync((void*)v.zero, 0, 256, c->stream));
  c->unet.zero_page_ready = true;
  return SH_OK;
}

// work tickets of a persistent launch: the next free counter of this forward pass and the table of item bounds (ticket_table) for the
// step's (items, workgroups, cout groups), built and uploaded once per shape
struct Tickets { unsigned* tk = nullptr; const int* tab = nullptr; int n = 0; };
static int take_tickets(sh_ctx* c, const UnetView& v, const UnetStep& s, Tickets* t) {
  sh_ctx::Unet& u = c->unet;
  const auto key = std::make_tuple(s.tk_items, s.tk_nwg, s.tk_ngrp);
  auto it = u.tk_tabs.find(key);
  if (it == u.tk_tabs.end()) {
    const std::vector<int> tab = ticket_table(s.tk_items, s.tk_nwg, s.tk_ngrp);
    if ((int)tab.size() > SH_UNET_TKTAB) return fail(c, SH_ERR_CAPACITY, "unet: ticket table larger than its buffer");
    if (u.tk_tab_used + (int)tab.size() > SH_UNET_TKTAB) {      // many different shapes (sh_unet_infer with varying n): start the cache over
      HIPCHK(c, hipStreamSynchronize(c->stream));                // (launches that read the old tables are done)
      u.tk_tabs.clear();
      u.tk_tab_used = 0;
    }
    HIPCHK(c, hipMemcpyAsync(v.tk_tab + u.tk_tab_used, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // `tab` is a local
    it = u.tk_tabs.emplace(key, std::make_pair(u.tk_tab_used, (int)tab.size() - 1)).first;
    u.tk_tab_used += (int)tab.size();
  }
  if (u.ticket_next >= SH_UNET_TICKETS) return fail(c, SH_ERR_CAPACITY, "unet: out of work counters");
  t->tk = v.tickets + u.ticket_next++;
  t->tab = v.tk_tab + it->second.first;
  t->n = it->second.second;
  return SH_OK;
}

// a launch on the persistent grid the plan sized: its work tickets (none: one workgroup per item), then `go`
template <typename F>
static int persistent_launch(sh_ctx* c, const UnetView& v, const UnetStep& s, F&& go) {
  Tickets t;
  if (s.tk_items) { const int rc = take_tickets(c, v, s, &t); if (rc != SH_OK) return rc; }
  return go(t);
}

// ---- the instantiation a step names: one line each -------------------------------------------------------------------------
#define PICK(a, b, c_, d, ...) if (s.t[0] == (a) && s.t[1] == (b) && s.t[2] == (c_) && s.t[3] == (d)) return (__VA_ARGS__)
static auto pick_f32(const UnetStep& s) -> decltype(&k_conv_mfma_f32<9, 4>) {
  PICK(9, 4, 0, 0, k_conv_mfma_f32<9, 4>); PICK(9, 2, 0, 0, k_conv_mfma_f32<9, 2>); PICK(1, 4, 0, 0, k_conv_mfma_f32<1, 4>); PICK(1, 2, 0, 0, k_conv_mfma_f32<1, 2>);
  return nullptr;
}
static auto pick_x3(const UnetStep& s) -> decltype(&k_conv_mfma_x3<9, 4>) {
  PICK(9, 2, UF_FIRST | UF_POOL, 0, k_conv_mfma_x3<9, 2, UF_FIRST | UF_POOL, 0>);      // enc0b with enc0a computed while its halo tile is staged
  PICK(9, 2, UF_HEAD, 1, k_conv_mfma_x3<9, 2, UF_HEAD>);      // (no pass plans it: the head stays on k_head; the library keeps the parent's kernels)
  PICK(9, 4, UF_POOL, 1, k_conv_mfma_x3<9, 4, UF_POOL>); PICK(9, 2, UF_POOL, 0, k_conv_mfma_x3<9, 2, UF_POOL, 0>);
  PICK(9, 4, 0, 1, k_conv_mfma_x3<9, 4>); PICK(9, 2, 0, 0, k_conv_mfma_x3<9, 2, 0, 0>); PICK(1, 4, 0, 1, k_conv_mfma_x3<1, 4>); PICK(1, 2, 0, 1, k_conv_mfma_x3<1, 2>);
  return nullptr;
}
static auto pick_x3r(const UnetStep& s) -> decltype(&k_upconv_x3r<2, 4>) {
  PICK(2, 4, 0, 0, k_upconv_x3r<2, 4>); PICK(4, 4, 0, 0, k_upconv_x3r<4, 4>); PICK(8, 2, 0, 0, k_upconv_x3r<8, 2>); PICK(16, 1, 0, 0, k_upconv_x3r<16, 1>);
  return nullptr;
}
template <int EK> static auto pick_conv16(const UnetStep& s) -> decltype(&k_conv_mfma16<EK, 9, 4, 0>) {
  PICK(9, 4, 0, 0, k_conv_mfma16<EK, 9, 4, 0>); PICK(9, 4, UF_POOL, 0, k_conv_mfma16<EK, 9, 4, UF_POOL>); PICK(9, 2, 0, 0, k_conv_mfma16<EK, 9, 2, 0>);
  PICK(1, 4, 0, 0, k_conv_mfma16<EK, 1, 4, 0>); PICK(1, 2, 0, 0, k_conv_mfma16<EK, 1, 2, 0>);
  return nullptr;
}
template <int EK> static auto pick_ldr16(const UnetStep& s) -> decltype(&k_conv3_ldr16<EK, 0, 0>) {
  PICK(UF_POOL, 1, 0, 0, k_conv3_ldr16<EK, UF_POOL, 1>); PICK(UF_POOL, 0, 0, 0, k_conv3_ldr16<EK, UF_POOL, 0>); PICK(0, 1, 0, 0, k_conv3_ldr16<EK, 0, 1>); PICK(0, 0, 0, 0, k_conv3_ldr16<EK, 0, 0>);
  return nullptr;
}
template <int EK> static auto pick_upg16(const UnetStep& s) -> decltype(&k_upconv16g<EK, 4, 4, 4, true>) {
  PICK(4, 4, 4, 1, k_upconv16g<EK, 4, 4, 4, true>); PICK(8, 2, 4, 1, k_upconv16g<EK, 8, 2, 4, true>); PICK(16, 2, 2, 0, k_upconv16g<EK, 16, 2, 2, false>);
  return nullptr;
}
#undef PICK
#define EK2(fn) (s.ek ? fn<1> : fn<0>)      // the bf16 / f16 pair of a 16-bit kernel or picker

// One step of the plan: its pointers from the view, its kernel from the plan's kind and template arguments.  A kernel the plan names
// and the library lacks is an error, never another kernel.
static int launch_step(sh_ctx* c, const UnetView& v, const UnetStep& s) {
  const char* nm = s.timer.c_str();
  const dim3 g(s.grid[0], s.grid[1], s.grid[2]), blk(s.block);
  const float *w = v.P + s.L.w_off, *b = v.P + s.L.b_off, *w2 = v.P + s.L2.w_off, *b2 = v.P + s.L2.b_off;      // (L2: the layer fused in)
  const u16* w16 = v.PW ? v.PW + s.L.w_off : nullptr;
  const int H = s.H, W = s.W, nimg = v.nimg;
  const size_t npx = (size_t)nimg * H * W;
  const float* nf = nullptr;
  const int missing = SH_ERR_STATE;
#define NEED(k) if (!(k)) return fail(c, missing, "unet: no kernel " + s.text() + " for " + s.timer)
  switch (s.kind) {
    case UK_CONV_FIRST: LAUNCH(c, nm, k_conv_first, g, blk, v.io.image, w, b, v.at<float>(s.dst), H, W, s.cout, nimg); break;
    case UK_CONV_FIRST16: LAUNCH(c, nm, EK2(k_conv_first16), g, blk, v.io.image, w, b, v.at<u16>(s.dst), H, W, s.cout, nimg); break;
    case UK_MAXPOOL2: LAUNCH(c, nm, k_maxpool2, g, blk, v.at<float>(s.src0), v.at<float>(s.dst), H, W, s.C0, nimg); break;
    case UK_MAXPOOL2_16: LAUNCH(c, nm, EK2(k_maxpool2_16), g, blk, v.at<u16>(s.src0), v.at<u16>(s.dst), H, W, s.C0, nimg); break;
    case UK_HEAD: LAUNCH(c, nm, (s.t[0] == 32 ? k_head<32> : k_head<64>), g, blk, v.at<float>(s.src0), w, b, v.io.logits, s.C0, npx); break;
    case UK_HEAD16: LAUNCH(c, nm, EK2(k_head16), g, blk, v.at<u16>(s.src0), w, b, v.io.logits, s.C0, npx, (size_t)H * W); break;
    case UK_CONV_F32: {
      const auto k = pick_f32(s);
      NEED(k);
      LAUNCH(c, nm, k, g, blk, v.at<float>(s.src0), v.at<float>(s.src1), s.C0, s.C1, w, b, v.at<float>(s.dst), H, W, s.cout, s.relu);
    } break;
    case UK_CONV_X3: {      // weights split once per parameter block (pack_weights)
      const auto k = pick_x3(s);
      NEED(k);
      const bool first = s.fuse & UF_FIRST, head = s.fuse & UF_HEAD;
      LAUNCH(c, nm, k, g, blk, v.at<float>(s.src0), v.at<float>(s.src1), s.C0, s.C1, v.wh + s.L.w_off, v.wl + s.L.w_off, b, v.at<float>(s.dst), H, W, s.cout, s.relu,
             v.at<float>(s.pool), head ? w2 : nf, head ? b2 : nf, head ? v.io.logits : nullptr, first ? v.io.image : nf, first ? w2 : nf, first ? b2 : nf);
    } break;
    case UK_UPCONV_X3R: {
      const auto k = pick_x3r(s);
      NEED(k);
      LAUNCH(c, nm, k, g, blk, v.at<float>(s.src0), v.wh + s.L.w_off, v.wl + s.L.w_off, b, v.at<float>(s.dst), H, W, s.cout);
    } break;
    case UK_CONV16: {
      const auto k = EK2(pick_conv16)(s);
      NEED(k);
      ConvFuse fz{};
      fz.pooled = v.at<u16>(s.pool);
      LAUNCH(c, nm, k, g, blk, v.at<u16>(s.src0), v.at<u16>(s.src1), s.C0, s.C1, w16, b, v.at<u16>(s.dst), H, W, s.cout, s.relu, fz);
    } break;
    case UK_CONV3_LDR16: {
      const auto k = EK2(pick_ldr16)(s);
      NEED(k);
      return persistent_launch(c, v, s, [&](const Tickets& t) -> int {
        LAUNCH(c, nm, k, g, blk, v.at<u16>(s.src0), v.at<u16>(s.src1), s.C0, s.C1, w16, b, v.at<u16>(s.dst), H, W, s.cout, s.relu, nimg, v.zero, v.at<u16>(s.pool), t.tk, t.tab, t.n);
        return SH_OK;
      });
    }
    case UK_UPCONV16G: {
      const auto k = EK2(pick_upg16)(s);
      NEED(k);
      return persistent_launch(c, v, s, [&](const Tickets& t) -> int {
        LAUNCH(c, nm, k, g, blk, v.at<u16>(s.src0), w16, b, v.at<u16>(s.dst), H, W, s.cout, nimg, t.tk, t.tab, t.n);
        return SH_OK;
      });
    }
    case UK_UPCONV16: LAUNCH(c, nm, EK2(k_upconv16), g, blk, v.at<u16>(s.src0), s.C0, w16, b, v.at<u16>(s.dst), H, W, s.cout); break;
    case UK_ENC0_PP:      // L2 = enc0a
      return persistent_launch(c, v, s, [&](const Tickets& t) -> int {
        LAUNCH_FN(c, nm, launch_enc0_pp(s.ek, g.x, c->stream, v.io.image, w2, b2, w16, b, v.at<u16>(s.dst), v.at<u16>(s.pool), H, W, nimg, v.io.raw, v.io.mm, t.tk, t.tab, t.n));
        return SH_OK;
      });
    case UK_DEC0A_UP_PP:      // L2 = up0
      return persistent_launch(c, v, s, [&](const Tickets& t) -> int {
        LAUNCH_FN(c, nm, launch_dec0a_up_pp(s.ek, g.x, c->stream, v.at<u16>(s.src0), v.at<u16>(s.src1), w16, b, v.PW + s.L2.w_off, b2, v.at<u16>(s.dst), H, W, nimg, v.zero, t.tk, t.tab, t.n));
        return SH_OK;
      });
    case UK_DEC0B_HEAD_PP:      // L2 = head
      return persistent_launch(c, v, s, [&](const Tickets& t) -> int {
        LAUNCH_FN(c, nm, launch_dec0b_head_pp(s.ek, g.x, c->stream, v.at<u16>(s.src0), w16, b, w2, b2, v.io.logits, H, W, nimg, v.zero, t.tk, t.tab, t.n));
        return SH_OK;
      });
    default: return fail(c, missing, "unet: no kernel " + s.text() + " for " + s.timer);
  }
#undef NEED
  return SH_OK;
}

namespace sh {
// One forward pass: plan, buffers, view, the steps.  The plan is built per call (tens of short strings and map lookups, as the walks
// it replaces did).
int unet_dispatch(sh_ctx* c, const UnetIO& io, int nimg, int H, int W) {
  const int dtype = c->params.unet_dtype;
  const bool b16 = unet_is16(dtype);
  std::vector<UnetStep> steps;
  const UnetError e = unet_plan(c->ulayers, c->pstate.shape().base, c->pstate.shape().depth, dtype, c->unet.reference, H, W, nimg, b16 ? persistent_grid(c) : 0, io.raw != nullptr, &steps);
  if (e.code != SH_OK) return fail(c, e.code, e.text);
  UnetView v;
  int rc;
  if ((rc = unet_view(c, io, nimg, H, W, &v)) != SH_OK) return rc;
  if (b16 || dtype == SH_UNET_F32X) { if ((rc = pack_weights(c, v, b16 ? (dtype == SH_UNET_F16) : -1)) != SH_OK) return rc; }
  if (b16) {
    if ((rc = zero_page(c, v)) != SH_OK) return rc;
    FILL(c, {v.tickets, (size_t)SH_UNET_TICKETS * 4, 0});
    c->unet.ticket_next = 0;
  }
  for (const UnetStep& s : steps)
    if ((rc = launch_step(c, v, s)) != SH_OK) return rc;
  return SH_OK;
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
  float *d_image = nullptr, *d_logits = nullptr;
  if ((rc = ensure(c, "infer.image", bytes, 4, (void**)&d_image)) != SH_OK) return rc;
  if ((rc = ensure(c, "infer.logits", bytes, 4, (void**)&d_logits)) != SH_OK) return rc;
  WindowScope whole(c, 0, c->Bwin);      // named buffers below are whole-batch
  HIPCHK(c, hipMemcpyAsync(d_image, images, bytes, hipMemcpyHostToDevice, c->stream));
  rc = unet_dispatch(c, {d_image, nullptr, nullptr, d_logits}, n, H, W);
  if (rc != SH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
  HIPCHK(c, hipMemcpyAsync(logits, d_logits, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

}  // extern "C"
