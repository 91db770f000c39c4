// Whole-model kernel schedule of the UNITER encoder: the library owns the
// sequence of launches for UniterModel.forward (model/model.py:336-367,
// BertLayer.forward model/layer.py:166-170) and for its backward, so the host
// makes a handful of calls per training step instead of ~60 framework
// dispatches per layer.
//
// Streams: the forward and the backward dgrad chain run on `stream`; weight /
// bias gradient GEMMs of layer l run on `side_stream` behind an event, so they
// overlap layer l-1's dgrad chain and fill the CUs that the partial last wave
// of each GEMM leaves idle.  Every layer owns its backward scratch, so the two
// streams never race on a buffer (288 GB of HBM: ~3 GB for UNITER-base B=16).
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "common.h"
#include "gemm_internal.h"
#include "philox.h"
#include "switches.h"

namespace {

enum { P_WORD = 0, P_POS, P_TYPE, P_ELN_G, P_ELN_B, P_IMG_W, P_IMG_B, P_ILN_G, P_ILN_B, P_PLN_G, P_PLN_B,
       P_POSL_W, P_POSL_B, P_MASK_EMB, P_FLN_G, P_FLN_B, P_LAYER0 };
enum { L_QW = 0, L_QB, L_KW, L_KB, L_VW, L_VB, L_OW, L_OB, L_LN1_G, L_LN1_B, L_W1, L_B1, L_W2, L_B2, L_LN2_G,
       L_LN2_B, L_COUNT };

const char* kEmbNames[P_LAYER0] = {
    "embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
    "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias",
    "img_embeddings.img_linear.weight", "img_embeddings.img_linear.bias",
    "img_embeddings.img_layer_norm.weight", "img_embeddings.img_layer_norm.bias",
    "img_embeddings.pos_layer_norm.weight", "img_embeddings.pos_layer_norm.bias",
    "img_embeddings.pos_linear.weight", "img_embeddings.pos_linear.bias",
    "img_embeddings.mask_embedding.weight", "img_embeddings.LayerNorm.weight", "img_embeddings.LayerNorm.bias"};
const char* kLayerNames[L_COUNT] = {
    "attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight",
    "attention.self.key.bias", "attention.self.value.weight", "attention.self.value.bias",
    "attention.output.dense.weight", "attention.output.dense.bias", "attention.output.LayerNorm.weight",
    "attention.output.LayerNorm.bias", "intermediate.dense.weight", "intermediate.dense.bias",
    "output.dense.weight", "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias"};

struct Carver {
  char* base; size_t off;
  explicit Carver(void* b) : base((char*)b), off(0) {}
  float* f(size_t n) { float* p = (float*)(base + off); off += align_up(n * sizeof(float), 256); return p; }
  unsigned short* h(size_t n) { unsigned short* p = (unsigned short*)(base + off); off += align_up(n * 2, 256); return p; }
  void* raw(size_t n) { void* p = base + off; off += align_up(n, 256); return p; }
};

struct LayerBufs {   // saved activations + backward scratch of one layer
  float *qkv, *lse, *ctx, *t1, *z1, *mean1, *rstd1, *y1, *u, *hact, *t2, *z2, *mean2, *rstd2, *y2;
  float *dz2, *g2, *du, *dy1, *dz1, *g1, *dctx, *dqkv, *delta, *dx, *du_csum;
  unsigned short* keepb;      // dropout keep flags of the attention probabilities (forward -> dQ)
  float* qb_part;             // [B, 3H] per-sample column sums of dqkv from the attention backward kernels
  void *ln_ws1, *ln_ws2;      // column partials of the two LayerNorm backward passes (finalized on the side stream)
  // precision 2: bf16 copies that feed the bf16-resident GEMMs (hact and du exist only in bf16 there)
  // precision 3: the same tensors as x3 pieces [rows][3][cols] (three times the elements) for the fp32-accurate products
  unsigned short *ctxb, *y1b, *hactb, *y2b, *g2b, *dub, *g1b, *dqkvb;
};

// How the encoder's dense products run (uniter_model_set_precision).  A forward pass copies the model's setting into its plan
// (make_plan); the schedule of that pass and of its backward pass reads the plan's copy only.
enum Precision {
  PREC_F32 = 0,         // fp32 MFMA GEMMs
  PREC_BF16_MFMA = 1,   // bf16 MFMA GEMMs on fp32 storage: scheduled like PREC_F32, gemm() picks the kernel
  PREC_BF16 = 2,        // bf16-resident operands: activations are handed on as bf16 copies, weights come from the bf16 mirror
  PREC_X3 = 3           // fp32 from three bf16 pieces per value: operand copies and mirror hold x3 pieces
};

// An activation as the dense products see it: its fp32 tensor and its operand copy (bf16 in PREC_BF16, x3 pieces [rows][3][cols] in
// PREC_X3, none below).  As an output: a product that is given a place for the operand copy writes ONLY that.
struct Act { float* f; unsigned short* b; };

struct Plan {
  int B, T, R, L, S, T0, M, mode;
  bool has_txt, has_img;
  bool gelu_d;      // forward stored gelu'(u) in LayerBufs::u rather than u
  // the attention kernels of this plan's forward and backward pass (attn_kernel(), decided once by uniter_model_forward)
  AttnKernel attn_fwd, attn_bwd;
  float *feat_eff, *imgfc, *img_stats, *cat, *emb;
  std::vector<LayerBufs> layers;
  float *dcat, *d_imgfc, *d_posfc, *d_feat, *dsum, *dpk;
  unsigned short* embb;   // precision 2: bf16 copy of the embedding output
  Precision prec = PREC_F32;   // what this plan was carved for: PREC_X3's *b buffers hold x3 pieces [rows][3][cols], embb likewise
  bool copies() const { return prec >= PREC_BF16; }      // activations have operand copies (LayerBufs::*b, embb)
  int ns_kh;              // precision 3: k-pieces of the attention-output forward product (N = K = hidden)
  // precision 3: k-pieces of the BACKWARD pass's N = hidden products (FFN-up / attention-output / QKV input gradients), chosen for the
  // CUs the backward pass may use: all of them, or what a data-parallel exchange leaves (uniter_model_set_cu_reserve)
  int ns_ki_b, ns_kh_b, ns_k3h_b;
  // precision 2: k-pieces of the GEMMs whose N is the hidden size (their fp32 outputs are that many slabs, summed by
  // the LayerNorm row pass that consumes them): K = intermediate (FFN-down forward, FFN-up dgrad), K = 3 hidden (QKV dgrad)
  int ns_ki, ns_k3h;
  bool packed;      // rows = valid positions only (uniter_batch_t::cu_seqlens)
  bool det;         // every sum of this plan's backward pass runs in a fixed order (uniter_model_set_deterministic when the plan was made):
                    // the embedding passes, the attention kernels' bias partials, the column sums, no stream-K dense product
  int wg_group;           // precision 2: the layer's four weight gradients as one whole-K-tile launch (0 = stream-K, 1 / 4 = LDS stages cfg)
  float* wg_slabs;        // precision 2: k-piece slabs of the split-K weight-gradient GEMMs (side stream, reused by every layer)
  unsigned char* hid_keepb;   // hidden-dropout keep flags of every layer's two sites, drawn ahead (round 5); stride hid_stride per site
  size_t hid_stride;
  bool hid_on;                // the forward pass drew them (this plan's row passes read them, forward and backward)
  void *ln_ws, *col_ws, *emb_ws, *attn_ws;
  void *emb_ws2, *emb_ws3;   // round 6: the text branch of the embedding backward and the region projection's bias column sums run on
                             // the auxiliary stream beside the image branch: partial-sum workspaces of their own
  size_t ln_ws_bytes, col_ws_bytes, emb_ws_bytes, attn_ws_bytes;
  // precision 3: workspaces of the balanced walk of the 128 x 256-tile products (gemm_split3.hip): one for the main stream's
  // launches, one for the weight-gradient stream's (they run at the same time); their flag words are cleared by every forward pass
  void *sk_main, *sk_side;
  size_t sk_bytes;
  // "head rows only" (uniter_model_set_head_rows), precision 3 on a padded batch: the last layer's stretch behind its attention kernel
  // on the B rows b * L alone.  hr: that stretch's buffers, B rows each with natural leading dimensions (hr.ctx / hr.ctxb: those rows of
  // the context, hr.dctx / hr.dz1: of the gradients the attention backward and the QKV input gradient read full-size, zero elsewhere);
  // hr_x / hr_dy: those rows of the layer's input and of the caller's gradient
  bool head_rows = false;     // this plan's forward pass ran that way: its backward pass does too
  // k-pieces of that stretch's N = hidden products by reduction length (hidden: attention output; intermediate: FFN-down forward, FFN-up
  // input gradient).  B rows are one row of tiles -- six workgroups at N = 768 -- so a product's time is its k-loop's: 1.1 us per
  // k-tile, 108 us at K = 3072 in one piece (measured); pieces of at least two k-tiles, eight at most, spread it over the chip and
  // the row pass behind sums the slabs (B rows each: nothing beside the k-loop they shorten)
  int hr_ns_h = 1, hr_ns_i = 1;
  LayerBufs hr;
  float *hr_x = nullptr, *hr_dy = nullptr;
  size_t total;
};

}  // namespace

struct uniter_model {
  uniter_config_t cfg;
  int n_params;
  std::vector<float*> p, g;
  std::vector<std::string> names;
  std::vector<hipEvent_t> ev_main, ev_side, ev_mid;
  Precision precision = PREC_F32;   // the caller's setting, any of the four modes; the schedule reads the copy in the plan (Plan::prec)
  bool mirror_paired = false;               // precision 3: the encoder layers' weights sit in the mirror in the paired-row layout
  const unsigned short* mirror = nullptr;   // bf16 copy of the flat parameter buffer (precision 2; precision 3: its three pieces)
  const float* mirror_base = nullptr;
  size_t mirror_numel = 0;
  const unsigned short* WB(int l, int k) const { return mirror + (LP(l, k) - mirror_base); }
  std::vector<hipEvent_t> ready;   // [embeddings, layer 0 .. nl-1]: parameters usable once the event has fired (consumed by the next forward)
  // profiling
  int prof_kind = 0;         // UNITER_K_* to time, or -1 = every kind
  std::vector<hipEvent_t> prof_ev;
  std::vector<int> prof_tag;     // kind of each recorded event pair
  size_t prof_used = 0;
  // in-kernel launch stamps of the GEMMs (uniter_prof_enable_stamps)
  unsigned long long* stamp_buf = nullptr;   // device: [cap][2][STAMP_WGS] = per-workgroup start / end, 100 MHz ticks
  size_t stamp_cap = 0, stamp_used = 0;
  std::vector<int> stamp_tag;
  // state carried from forward to backward
  Plan plan;
  uniter_batch_t batch;
  float* hidden_out = nullptr;
  const float* d_hidden = nullptr;
  int all_layers = 0;
  uint64_t seed = 0;
  uint32_t offset = 0;
  hipStream_t st = nullptr, side = nullptr;
  bool bwd_open = false;
  bool deterministic = false;     // uniter_model_set_deterministic: the plans made from now on run order-fixed (Plan::det)
  int cu_reserve = 0;             // uniter_model_set_cu_reserve: CUs the persistent launches of this model's backward pass leave free
  int launch_reserve = 0;         // ... and of the pass that is running: 0 from uniter_model_forward on (no collective of the step is in flight
                                  // during its forward pass), cu_reserve from the backward calls on -- LaunchOpts::cu_reserve of every launch
  hipStream_t aux = nullptr;      // uniter_model_set_aux_stream: launches that depend on nothing the step computes (dropout keep flags)
  hipEvent_t ev_aux0 = nullptr, ev_aux1 = nullptr, ev_aux2 = nullptr;
  hipEvent_t ev_emb0 = nullptr, ev_emb1 = nullptr, ev_emb2 = nullptr;      // embedding backward: main <-> auxiliary stream
  double* norm_parts = nullptr;   // uniter_model_set_norm_partials: layer l's clip-norm partial sums at norm_parts + l * norm_stride
  size_t norm_stride = 0;
  bool wg_overwrite = false; // the next backward pass overwrites the encoder's weight gradients (uniter_model_set_wgrad_overwrite)
  // uniter_model_set_input_grads: the perturbation the next forward pass reads and the input gradients its backward pass writes
  struct InputGrads { const float* txt_delta = nullptr; float* d_txt_rows = nullptr; float* d_img_feat = nullptr; float* d_img_pos_feat = nullptr;
                      bool outputs() const { return d_txt_rows || d_img_feat || d_img_pos_feat; } };
  InputGrads ig_next, ig;    // as set / as the latest forward pass took it over (its backward pass reads ig)
  // uniter_model_set_attn_probs: where the next forward pass leaves every layer's attention probabilities (out == nullptr: nowhere)
  struct AttnProbs { float* out = nullptr; size_t stride = 0; int head_mean = 0; };
  AttnProbs ap_next;
  bool head_rows_next = false;   // uniter_model_set_head_rows: the next forward pass's (Plan::head_rows is what that pass made of it)
  // uniter_model_set_attn_grads: where the backward pass of the next forward pass leaves every layer's gradient-weighted attention
  // (out == nullptr: nowhere)
  struct AttnGrads { float* out = nullptr; size_t stride = 0; int reduce = 0; float* head_sums = nullptr; void* ws = nullptr; size_t ws_bytes = 0; };
  AttnGrads ag_next, ag;     // as set / as the latest forward pass took it over (its backward pass reads ag)
  uint64_t generation = 0;   // bumped by every forward: a backward must belong to the LATEST forward (one plan / workspace per model)

  float* P(int i) const { return p[i]; }
  float* G(int i) const { return g[i]; }
  float* LP(int l, int k) const { return p[P_LAYER0 + l * L_COUNT + k]; }
  float* LG(int l, int k) const { return g[P_LAYER0 + l * L_COUNT + k]; }
  int pooler_w() const { return P_LAYER0 + cfg.num_hidden_layers * L_COUNT; }
};

namespace {

int check_cfg(const uniter_config_t* c) {
  UCHECK_ARG(c, "config is NULL");
  UCHECK_SHAPE(c->hidden_size > 0 && c->num_attention_heads > 0 &&
               c->hidden_size == 64 * c->num_attention_heads,
               "hidden_size (%d) must be 64 * num_attention_heads (%d): head_dim 64 only", c->hidden_size,
               c->num_attention_heads);
  UCHECK_SHAPE(c->hidden_size <= 1024, "hidden_size %d > 1024 unsupported", c->hidden_size);
  UCHECK_SHAPE(c->intermediate_size % 4 == 0 && c->img_dim % 4 == 0, "intermediate_size / img_dim must be multiples of 4");
  UCHECK_SHAPE(c->num_hidden_layers >= 1 && c->vocab_size > 0 && c->max_position_embeddings > 0 &&
               c->type_vocab_size >= 2, "bad config");
  return 0;
}

int x3_backward_cus(const uniter_model* m);

void make_plan(const uniter_model* m, Plan& pl, void* ws, int B, int T, int R, int L, bool has_txt,
               bool has_img, bool has_masks, int mode, int Mrows = -1) {
  const uniter_config_t& c = m->cfg;
  const Switches& sw = uniter_switches();
  const int H = c.hidden_size, I = c.intermediate_size, nl = c.num_hidden_layers, nh = c.num_attention_heads;
  pl.B = B; pl.T = T; pl.R = R; pl.L = L; pl.mode = mode; pl.has_txt = has_txt; pl.has_img = has_img;
  pl.T0 = has_txt ? T : 0;
  pl.S = pl.T0 + (has_img ? R : 0);
  pl.packed = Mrows >= 0;
  pl.det = false;
  pl.M = pl.packed ? Mrows : B * L;
  const size_t M = (size_t)pl.M;
  Carver cv(ws);
  const size_t BR = (size_t)B * (has_img ? R : 0);
  pl.feat_eff = has_masks ? cv.f(BR * c.img_dim) : nullptr;
  pl.imgfc = cv.f(BR * H);
  pl.img_stats = cv.f(BR * 6);
  pl.cat = cv.f((size_t)B * pl.S * H);
  pl.emb = cv.f(M * H);
  pl.prec = m->precision;
  const bool res = pl.prec == PREC_BF16, x3 = pl.prec == PREC_X3;
  pl.hid_keepb = nullptr; pl.hid_stride = 0; pl.hid_on = false;
  const size_t pc = x3 ? 3 : 1;       // bf16 elements per value in the operand copies
  // The plan is made by the forward pass, which reserves no CU (uniter_model_forward: launch_reserve = 0), and sized ahead of it by
  // uniter_model_ws_bytes, which must carve the same plan whatever pass ran last on the handle: the forward products' k-pieces are
  // chosen for the whole chip, the backward pass's (x3) for x3_backward_cus.
  const int fwd_reserve = 0;
  pl.embb = pl.copies() ? cv.h(pc * M * H) : nullptr;
  pl.ns_ki = res ? gemm_bf16v2_pick_split(pl.M, H, I) : x3 ? gemm_x3_pick_split(pl.M, H, I) : 1;
  pl.ns_k3h = res ? gemm_bf16v2_pick_split(pl.M, H, 3 * H) : x3 ? gemm_x3_pick_split(pl.M, H, 3 * H) : 1;
  if (res && (sw.b16_persist & 2)) {
    // round 6: the N = hidden products on the persistent kernels are planned by their own cost model (one workgroup per CU: two
    // k-pieces fill the chip where gemm_dma_kernel's two workgroups per CU wanted four -- two slabs less for the row pass behind)
    const int a = gemm_b1p_pick_split(pl.M, H, I, 0, fwd_reserve), b = gemm_b1p_pick_split(pl.M, H, 3 * H, 0, fwd_reserve);
    if (a > 1) pl.ns_ki = a;
    if (b > 1) pl.ns_k3h = b;
  }
  pl.ns_kh = x3 ? gemm_x3_pick_split(pl.M, H, H) : 1;
  pl.ns_ki_b = pl.ns_ki; pl.ns_k3h_b = pl.ns_k3h; pl.ns_kh_b = pl.ns_kh;
  if (x3) {
    // (the forward pass runs before any collective of its step: it keeps every CU; the backward pass's products are planned for the
    // CUs it will have)
    const int avail_b = x3_backward_cus(m);
    pl.ns_ki = gemm_x3_pick_split_on(pl.M, H, I, 0, fwd_reserve); pl.ns_kh = gemm_x3_pick_split_on(pl.M, H, H, 0, fwd_reserve);
    pl.ns_ki_b = gemm_x3_pick_split_on(pl.M, H, I, avail_b, 0);      // (avail_b > 0 is the CU count: no reserve on top of it)
    pl.ns_kh_b = gemm_x3_pick_split_on(pl.M, H, H, avail_b, 0);
    pl.ns_k3h_b = pl.ns_k3h = gemm_x3_pick_split_on(pl.M, H, 3 * H, avail_b, 0);
  }
  const size_t s_ki = (size_t)pl.ns_ki, s_k3h = (size_t)pl.ns_k3h, s_kh = (size_t)pl.ns_kh;
  const size_t s_ki_b = (size_t)pl.ns_ki_b, s_kh_b = (size_t)pl.ns_kh_b;
  pl.layers.resize(nl);
  const bool save = mode != 0;
  auto alloc_fwd = [&](LayerBufs& b) {
    b.qkv = cv.f(M * 3 * H); b.lse = cv.f((size_t)B * nh * L); b.ctx = cv.f(M * H); b.t1 = cv.f(s_kh * M * H);
    b.z1 = save ? cv.f(M * H) : nullptr; b.mean1 = cv.f(M); b.rstd1 = cv.f(M); b.y1 = cv.f(M * H);
    b.u = save ? cv.f(M * I) : nullptr; b.hact = cv.f(M * I); b.t2 = cv.f(s_ki * M * H);
    b.z2 = save ? cv.f(M * H) : nullptr; b.mean2 = cv.f(M); b.rstd2 = cv.f(M); b.y2 = cv.f(M * H);
    if (pl.copies()) { b.ctxb = cv.h(pc * M * H); b.y1b = cv.h(pc * M * H); b.hactb = cv.h(pc * M * I); b.y2b = cv.h(pc * M * H); }
  };
  if (save) {
    for (int l = 0; l < nl; ++l) {
      LayerBufs& b = pl.layers[l];
      b = LayerBufs();
      alloc_fwd(b);
      b.dz2 = cv.f(M * H); b.g2 = cv.f(M * H); b.du = cv.f(M * I); b.dy1 = cv.f(s_ki_b * M * H); b.dz1 = cv.f(M * H);
      b.g1 = cv.f(M * H); b.dctx = cv.f(s_kh_b * M * H); b.dqkv = cv.f(M * 3 * H); b.delta = cv.f((size_t)B * nh * L);
      b.dx = cv.f(s_k3h * M * H);
      b.du_csum = cv.f((size_t)((M + 31) / 32) * I);
      b.qb_part = cv.f((size_t)B * 3 * H);
      b.keepb = (unsigned short*)cv.raw(uniter_attn_keep_bits_bytes(B, L, nh));
      b.ln_ws1 = cv.raw(uniter_ln_bwd_ws_bytes(pl.M, H));
      b.ln_ws2 = cv.raw(uniter_ln_bwd_ws_bytes(pl.M, H));
      if (pl.copies()) { b.g2b = cv.h(pc * M * H); b.dub = cv.h(pc * M * I); b.g1b = cv.h(pc * M * H); b.dqkvb = cv.h(pc * M * 3 * H); }
    }
  } else {
    // inference: every layer reuses one set of buffers; the layer output ping-pongs
    LayerBufs base = LayerBufs();
    alloc_fwd(base);
    float* yB = cv.f(M * H);
    for (int l = 0; l < nl; ++l) {
      pl.layers[l] = base;
      if (l & 1) pl.layers[l].y2 = yB;
    }
  }
  // the balanced walk's workspaces (UNITER_X3_BALANCED, default off: bit 0 = the grouped weight gradients, bit 1 = the forward products)
  pl.sk_bytes = gemm_x3_sk_ws_bytes();
  pl.sk_main = (x3 && (sw.x3_balanced & 2)) ? cv.raw(pl.sk_bytes) : nullptr;
  pl.sk_side = (x3 && save && (sw.x3_balanced & 1)) ? cv.raw(pl.sk_bytes) : nullptr;
  pl.head_rows = false;
  pl.hr = LayerBufs(); pl.hr_x = pl.hr_dy = nullptr;
  if (x3 && !pl.packed) {      // (wherever a forward pass may honour uniter_model_set_head_rows: B rows of everything behind the attention kernel)
    const size_t Bc = (size_t)B;
    LayerBufs& h = pl.hr;
    auto pieces_for = [](int K) { const int n = K / 32 / 2; return n < 1 ? 1 : (n > 8 ? 8 : n); };
    pl.hr_ns_h = pieces_for(H); pl.hr_ns_i = pieces_for(I);
    const size_t s_h = (size_t)pl.hr_ns_h, s_i = (size_t)pl.hr_ns_i;
    h.ctx = cv.f(Bc * H); h.ctxb = cv.h(pc * Bc * H); pl.hr_x = cv.f(Bc * H); h.t1 = cv.f(s_h * Bc * H);
    h.z1 = save ? cv.f(Bc * H) : nullptr; h.mean1 = cv.f(Bc); h.rstd1 = cv.f(Bc); h.y1 = cv.f(Bc * H); h.y1b = cv.h(pc * Bc * H);
    h.u = save ? cv.f(Bc * I) : nullptr; h.hact = cv.f(Bc * I); h.hactb = cv.h(pc * Bc * I); h.t2 = cv.f(s_i * Bc * H);
    h.z2 = save ? cv.f(Bc * H) : nullptr; h.mean2 = cv.f(Bc); h.rstd2 = cv.f(Bc); h.y2 = cv.f(Bc * H);
    if (save) {
      pl.hr_dy = cv.f(Bc * H); h.dz2 = cv.f(Bc * H); h.g2b = cv.h(pc * Bc * H); h.dub = cv.h(pc * Bc * I); h.dy1 = cv.f(s_i * Bc * H);
      h.dz1 = cv.f(Bc * H); h.g1b = cv.h(pc * Bc * H); h.dctx = cv.f(Bc * H);
      h.du_csum = cv.f((size_t)((Bc + 31) / 32) * I);
      h.ln_ws1 = cv.raw(uniter_ln_bwd_ws_bytes(B, H));
      h.ln_ws2 = cv.raw(uniter_ln_bwd_ws_bytes(B, H));
    }
  }
  if (save) {
    pl.hid_stride = align_up(uniter_hidden_keep_bits_bytes(M * H), 256);
    pl.hid_keepb = (unsigned char*)cv.raw(pl.hid_stride * 2 * nl);
    pl.dcat = cv.f((size_t)B * pl.S * H);
    pl.d_imgfc = cv.f(BR * H);
    pl.d_posfc = cv.f(BR * H);
    pl.d_feat = has_masks ? cv.f(BR * c.img_dim) : nullptr;
    pl.dsum = cv.f(M * H);
    pl.dpk = cv.f(M * H);          // packed mode: d_hidden gathered to the valid rows
    pl.ln_ws_bytes = uniter_ln_bwd_ws_bytes(pl.M, H);
    pl.ln_ws = cv.raw(pl.ln_ws_bytes);
    const int maxN = 3 * H > I ? 3 * H : I;
    pl.col_ws_bytes = uniter_colsum_ws_bytes(pl.M, maxN);
    pl.col_ws = cv.raw(pl.col_ws_bytes);
    const int rows = B * (T > R ? T : R);
    pl.emb_ws_bytes = uniter_embed_bwd_ws_bytes(rows, H);
    pl.det = m->deterministic;
    if (pl.det) {     // emb_ws / emb_ws2 hold the order-fixed passes' per-row gradients, ranks and chunk sums as well
      const size_t d = uniter_embed_bwd_det_ws_bytes(has_txt ? B * T : 0, (int)BR, H);
      if (d > pl.emb_ws_bytes) pl.emb_ws_bytes = d;
    }
    pl.emb_ws = cv.raw(pl.emb_ws_bytes);
    pl.emb_ws2 = cv.raw(pl.emb_ws_bytes);
    pl.emb_ws3 = cv.raw(pl.emb_ws_bytes);
    pl.attn_ws_bytes = uniter_attn_bwd_ws_bytes(B, L, c.num_attention_heads);
    pl.attn_ws = cv.raw(pl.attn_ws_bytes);
    pl.wg_slabs = res ? cv.f((size_t)4 * 3 * H * (I > 3 * H ? I : 3 * H)) : nullptr;
    const int wg_env = sw.wgrad_group;      // (1, the default: one launch of whole-K tiles; 2 / 4: its measured-slower forms; 0: stream-K)
    pl.wg_group = (res && H % 8 == 0 && I % 8 == 0 && (wg_env == 1 || wg_env == 2 || wg_env == 4)) ? wg_env : 0;
    // the grouped kernel addresses its operands with 31-bit buffer offsets: very long batches keep the stream-K launches
    if ((size_t)(M + 64) * (I > 3 * H ? I : 3 * H) * 2 >= (1ull << 31)) pl.wg_group = 0;
  }
  pl.total = cv.off;
}

struct ProfScope {
  uniter_model* m; hipStream_t st; bool on;
  unsigned long long* stamp = nullptr;      // the stamp slot this scope reserved for the GEMM launched inside it (LaunchOpts::stamp), or none
  ProfScope(uniter_model* m_, int kind, hipStream_t st_) : m(m_), st(st_), on(false) {
    if (m->stamp_buf && kind && kind != UNITER_K_ATTN_FWD && kind != UNITER_K_ATTN_BWD && kind != UNITER_K_LN &&
        kind != UNITER_K_LN_BWD && m->stamp_used < m->stamp_cap) {
      m->stamp_tag[m->stamp_used] = kind;                     // the GEMM launched inside this scope is given the slot
      stamp = m->stamp_buf + (size_t)2 * STAMP_WGS * m->stamp_used++;
    }
    if (m->prof_kind && kind && (m->prof_kind == kind || m->prof_kind < 0) && m->prof_used + 2 <= m->prof_ev.size()) {
      on = true;
      m->prof_tag[m->prof_used / 2] = kind;
      hipEventRecord(m->prof_ev[m->prof_used], st);
    }
  }
  ~ProfScope() {
    if (on) { hipEventRecord(m->prof_ev[m->prof_used + 1], st); m->prof_used += 2; }
  }
};

int gemm(uniter_model* m, int kind, hipStream_t st, int akm, int bkm, int M, int N, int K, const float* A,
         int lda, const float* B, int ldb, float* C, int ldc, int epi, const float* bias, const float* aux_in,
         float* aux_out, int ld_aux, int beta, float* colsum_part = nullptr) {
  ProfScope ps(m, kind, st);
  const Switches& sw = uniter_switches();
  int cfg = 0;
  const bool wgrad = kind == UNITER_K_GEMM_WGRAD && akm && bkm && (beta == 1 || beta == -1);
  const Precision prec = m->plan.prec;
  // a deterministic plan never takes the stream-K form of a C += (float atomics in arrival order): whole tiles, one adder per element
  const int no_sk = m->plan.det ? 1 : 0;
  if (wgrad && (prec == PREC_F32 || prec == PREC_X3)) {
    // a layer's weight gradients by output shape: whole-K tiles (cfg 25, UNITER_WGRAD_WHOLE's bit) or UNITER_WGRAD_CFG's stream-K tiles
    cfg = sw.wgrad_cfg;
    const int H_ = m->cfg.hidden_size, I_ = m->cfg.intermediate_size;
    const int bit = (M == H_ && N == I_) ? 1 : (M == I_ && N == H_) ? 2 : (M == H_ && N == H_) ? 4 : (M == 3 * H_ && N == H_) ? 8 : 0;
    if (sw.wgrad_whole & bit) cfg = 25;
  }
  if (beta == -1) {
    // overwrite requested (uniter_model_set_wgrad_overwrite): whole-K tiles store their result; every form that adds
    // partial tiles with float atomics gets a cleared output first
    if (cfg == 25) beta = 0;
    else { UCHECK_HIP(hipMemsetAsync(C, 0, (size_t)M * ldc * sizeof(float), st)); beta = 1; }
  }
  // wave priority of the critical path's GEMMs over the side stream's weight gradients (common.h; UNITER_MAIN_PRIO, default 0)
  const LaunchOpts lo = {ps.stamp, kind == UNITER_K_GEMM_WGRAD ? 0 : sw.main_prio, m->launch_reserve};
  GemmCall c;
  c.M = M; c.N = N; c.K = K; c.A = {A, lda, 0, akm}; c.B = {B, ldb, 0, bkm}; c.C = C; c.ldc = ldc;
  c.epi = epi; c.bias = bias; c.aux_in = aux_in; c.aux_out = aux_out; c.ld_aux = ld_aux;
  c.beta = beta; c.no_sk = no_sk; c.colpart = colsum_part; c.stream = st;
  if (prec == PREC_BF16_MFMA || prec == PREC_BF16)      // embeddings' projections (fp32 inputs) also run on the bf16 pipe in mode 2
    return gemm_bf16_run(0, c, lo);
  return gemm_f32_run(cfg, kind == UNITER_K_GEMM_FFN_UP_FWD, c, lo);
}

// One dense product of encoder layer l against weight w (L_QW, L_OW, L_W1, L_W2): c = epilogue(a . W^T), or with b_kmajor the input
// gradient c = epilogue(a . W).  The site states the product; the plan's precision decides the operand format:
//   PREC_F32 / PREC_BF16_MFMA: fp32 operands and the fp32 weight, through gemm().
//   PREC_BF16: both operands already bf16 in memory (a's copy, the mirror's weight) on the LDS-DMA kernel (gemm_bf16_dma.hip); the
//     gelu' operand of the GELU epilogues (aux_out forward, aux_in of dU) is bf16 there, residual gradients fp32.
//   PREC_X3: a = x3 activations [M][3][K], W = the piece-major x3 mirror (piece stride = the flat parameter buffer's length), output
//     fp32 or x3 [M][3][N], aux operands fp32 (gemm_split3.hip).
// The fp32 output is `pieces` k-piece slabs [M][N], summed by the row pass or attention kernel that reads them.
int linear(uniter_model* m, int kind, hipStream_t st, int bkm, int M, int N, int K, int l, int w, Act a, Act c, int pieces, int epi,
           const float* bias, const float* aux_in, float* aux_out, float* colpart = nullptr) {
  const Plan& pl = m->plan;
  const Switches& sw = uniter_switches();
  const int ldw = bkm ? N : K;                                                        // W is [N][K] forward, [K][N] for an input gradient
  const int ld_aux = (epi == UNITER_EPI_NONE || epi == UNITER_EPI_BIAS) ? 0 : N;      // (the other epilogues read or write an [M][N] operand)
  float* C = c.b ? nullptr : c.f;
  if (!pl.copies()) {
    UCHECK_ARG(pieces == 1, "linear: the fp32 kernels write one slab");
    return gemm(m, kind, st, 0, bkm, M, N, K, a.f, K, m->LP(l, w), ldw, C, N, epi, bias, aux_in, aux_out, ld_aux, 0, colpart);
  }
  ProfScope ps(m, kind, st);
  GemmCall g;      // what every operand format shares: the weight from the mirror, `pieces` fp32 slabs or the operand-format copy
  g.M = M; g.N = N; g.K = K; g.B = {m->WB(l, w), ldw, 0, bkm}; g.C = C; g.ldc = N; g.c_split_stride = (long)M * N; g.nsplit = pieces;
  g.Ccopy = c.b; g.epi = epi; g.bias = bias; g.aux_in = aux_in; g.aux_out = aux_out; g.colpart = colpart; g.stream = st;
  if (pl.prec == PREC_X3) {
    const int cfg = (kind == UNITER_K_GEMM_FFN_UP_FWD && sw.x3_cfg_ffn_up_fwd) ? sw.x3_cfg_ffn_up_fwd : sw.x3_cfg;
    const LaunchOpts lo = {ps.stamp, sw.main_prio_x3, m->launch_reserve};
    g.A = {a.b, 3 * K, K, 0}; g.B.piece_stride = (int)m->mirror_numel; g.ld_copy = 3 * N; g.ps_copy = N; g.ld_aux = N;
    // (every product of this helper runs on the main stream: the balanced walk's main-stream workspace)
    g.sk_ws = pl.sk_main; g.sk_ws_bytes = pl.sk_main ? pl.sk_bytes : 0;
    // (cfg | 64: the weight's pieces in the paired-row layout -- full 128-byte source lines for the loaders of the forward products)
    return gemm_x3_run(cfg | (m->mirror_paired ? 64 : 0), g, lo);
  }
  const LaunchOpts lo = {ps.stamp, sw.main_prio_bf16, m->launch_reserve};
  g.A = {a.b, K, 0, 0}; g.ld_copy = c.b ? N : 0; g.ld_aux = ld_aux;
  g.aux_in_bf16 = epi == UNITER_EPI_MUL || epi == UNITER_EPI_DGELU; g.aux_out_bf16 = epi == UNITER_EPI_BIAS_GELU || epi == UNITER_EPI_BIAS_GELU_D;
  // round 6: the persistent loader / compute kernels (csrc/gemm_bf16_p.hip) for the products UNITER_B16_PERSIST names (default: none):
  // 1 = QKV forward, 2 = N = hidden products, 8 = the wide products as well (4: the grouped weight gradients, wgrad_group())
  int cfg = 0;
  const int mask = sw.b16_persist;
  const bool epi_ok = epi == UNITER_EPI_NONE || epi == UNITER_EPI_BIAS || epi == UNITER_EPI_ADD || epi == UNITER_EPI_BIAS_GELU_D || epi == UNITER_EPI_MUL;
  if (epi_ok && K % 64 == 0) {
    if ((mask & 1) && kind == UNITER_K_GEMM_QKV_FWD && !bkm && N % 192 == 0) cfg = 8;
    else if ((mask & 2) && pieces > 1 && N <= 1024) cfg = 6;
    else if ((mask & 8) && pieces == 1 && N >= 2048) cfg = 7;
  }
  if (colpart) {      // (the product that writes dU also leaves its column partials: the persistent 128 x 256 kernel's epilogue)
    UCHECK_ARG(epi_ok && K % 64 == 0 && pieces == 1, "linear: column partials ride on the persistent kernels");
    return gemm_b1p_run(7, g, lo);
  }
  return gemm_bf16v2_run(cfg, g, lo);
}
// The attention kernel of a plan's forward pass (`keep_pre`: the forward drew the dropout keep flags ahead of its kernels) or of its
// backward pass (bwd).  The kernels of attention_x3.hip (ATTN_X3, ATTN_B16X) read the keep flags and draw none, so with dropout they
// need them ready; the backward pass of a saved plan always finds them -- whichever forward kernel ran left them -- which is why a
// forward pass without pre-drawn flags (UNITER_KEEP_PREGEN=0) pairs a *_PRE forward kernel with the ATTN_X3 / ATTN_B16X backward.
AttnKernel attn_kernel(const Plan& pl, float p_drop, bool save, bool keep_pre, bool bwd) {
  const Switches& sw = uniter_switches();
  const bool fused = pl.L <= uniter_attn_varlen_max_len();      // the L <= 192 kernels (none with UNITER_ATTN_SPLIT=0)
  const bool pieces = pl.L <= uniter_attn_x3_max_len() && (p_drop == 0.f || keep_pre || bwd);
  // precision 2, L <= 192: attention on the bf16 pipe, which also writes the bf16 copies of its outputs
  if (pl.prec == PREC_BF16 && fused) return (sw.attn_b16x && pieces) ? ATTN_B16X : ATTN_BF16_PRE;
  // precision 3: the attention's own products on the bf16 pipe as well (its backward emits the fused query|key|value bias partials)
  if (pl.prec == PREC_X3 && sw.attn_x3 && pieces && (fused || !bwd)) return ATTN_X3;
  if (pl.prec == PREC_X3 && fused) return ATTN_F32_PRE_X3;
  if (pl.packed || (save && fused)) return ATTN_F32_PRE;
  return ATTN_F32;
}
// CUs the backward pass's persistent launches may use: the chip's minus what the caller reserved for a gradient exchange
int x3_backward_cus(const uniter_model* m) {
  const int a = (gemm_chip_cus() - m->cu_reserve) / 8 * 8;
  return a >= 8 ? a : 8;
}
// The grouped weight-gradient launch of layer l's backward pass (precision 2 or 3: four products, Mo = {I, H, 3H, H}, No = {H, I, H, H}):
// what rides on it, its geometry, its grid cap, and -- with riders -- the clip-norm slots it fills.  Read by backward_layer, which
// launches it, and by uniter_model_norm_partials_per_layer, which announces its slots.  cu_reserve: CUs the launch leaves free.
struct WgradGroup {
  bool riders = false;    // the layer's column reductions, intermediate.dense's bias gradient and its clip-norm share ride on the launch
  bool colpart = false;   // ... and dU's column sums (that bias gradient) start as column partials of the product that writes dU
  int cfg = 0, max_wgs = 0, slots = 0;
};
// own_k: the launch's products have reduction lengths of their own (a last layer on its head rows): no balanced walk, whose runs of
// k-tiles want one length
WgradGroup wgrad_group(const uniter_model* m, const Plan& pl, int l, int cu_reserve, bool own_k = false) {
  const Switches& sw = uniter_switches();
  const int H = m->cfg.hidden_size, I = m->cfg.intermediate_size;
  const int Mo[4] = {I, H, 3 * H, H}, No[4] = {H, I, H, H};
  WgradGroup g;
  if (pl.prec == PREC_X3) {
    // UNITER_X3_RIDERS, and the default geometries only.  Column partials whenever the launch runs on 128 x 256 tiles
    g.riders = sw.x3_riders && (sw.x3_cfg == 0 || sw.x3_cfg == 3);
    g.colpart = g.riders && gemm_x3_wgrad_default_cfg() == 4;
    g.cfg = g.riders ? (sw.x3_cfg == 3 ? 3 : 0) : sw.x3_cfg;
    // UNITER_WGRAD_X3_WGS = n forces a grid for every layer (0 = one workgroup per CU); unset, layer 0 takes the smallest grid that
    // needs no more rounds (switches.h) and every other layer one workgroup per CU
    g.max_wgs = sw.wgrad_x3_wgs >= 0 ? sw.wgrad_x3_wgs : (l == 0 ? gemm_x3_wgrad_group_balanced_wgs(0, 4, Mo, No, cu_reserve) : 0);
    if (g.riders) g.slots = gemm_x3_wgrad_group_slots(0, 4, Mo, No, g.max_wgs, pl.M, (pl.sk_side && !own_k) ? pl.sk_bytes : 0, cu_reserve);
    return g;
  }
  // precision 2: riders only on UNITER_B16_RIDERS=1 -- except with the launch on the persistent 128 x 256-tile kernel (UNITER_B16_PERSIST
  // bit 4), where they are on unless UNITER_B16_RIDERS=0 (switches.h)
  const bool p7 = (sw.b16_persist & 4) != 0;
  // (on the 128 x 256 geometry the bias gradient of intermediate.dense must come from column partials -- bit 8 and the gelu' form of the
  // forward epilogue: a separate pass over dU would write it outside the launch, and its squares would reach no clip-norm slot)
  g.riders = pl.wg_group == 1 && (p7 ? sw.b16_riders != '0' && (sw.b16_persist & 8) && pl.gelu_d : sw.b16_riders == '1');
  // ... finished by a fourth reduction job of the riders
  g.colpart = p7 && g.riders;
  g.cfg = pl.wg_group == 4 ? 4 : (p7 ? 7 : 1);      // (4: three LDS stages; 7: 216 whole-K tiles of 128 x 256 on the persistent kernel)
  g.max_wgs = 0;                                   // (the grid cap of UNITER_WGRAD_GROUP_WGS / its default)
  if (g.riders) g.slots = p7 ? gemm_b1p_wgrad_group_slots(4, Mo, No, g.max_wgs, cu_reserve) : gemm_bf16v2_wgrad_group_slots(4, Mo, No, g.max_wgs, cu_reserve);
  return g;
}
// the side work of layer l's backward as riders of its grouped weight-gradient launch (product 0 must be dW1 = dU^T y1: its A
// operand's column sums are intermediate.dense's bias gradient)
void fill_layer_riders(uniter_x3_riders_t& x, const uniter_model* m, int l, const LayerBufs& lb, int M, int B, int H, bool fused_qb,
                       bool colpart = false) {
  x.colsum_out = colpart ? nullptr : m->LG(l, L_B1);
  const int lnp = ln_bwd_partial_rows(M);
  x.njobs = fused_qb ? 3 : 2;
  x.part[0] = (const float*)lb.ln_ws2; x.part[1] = (const float*)lb.ln_ws1; x.part[2] = lb.qb_part;
  x.nparts[0] = x.nparts[1] = lnp; x.nparts[2] = B;
  x.stride[0] = x.stride[1] = x.stride[2] = 3 * H;
  x.n[0] = x.n[1] = x.n[2] = 3 * H;
  x.seg[0] = x.seg[1] = H; x.seg[2] = 3 * H;
  x.out[0][0] = m->LG(l, L_LN2_G); x.out[0][1] = m->LG(l, L_LN2_B); x.out[0][2] = m->LG(l, L_B2);
  x.out[1][0] = m->LG(l, L_LN1_G); x.out[1][1] = m->LG(l, L_LN1_B); x.out[1][2] = m->LG(l, L_OB);
  x.out[2][0] = m->LG(l, L_QB);
  if (!fused_qb) {      // (no per-sample query|key|value partials: the column-partial job, if any, takes slot 2)
    x.part[2] = nullptr; x.out[2][0] = nullptr;
  }
  if (colpart) {
    const int j = x.njobs++, I = m->cfg.intermediate_size;
    x.part[j] = lb.du_csum; x.nparts[j] = (M + 63) / 64; x.stride[j] = I; x.n[j] = I; x.seg[j] = I;
    x.out[j][0] = m->LG(l, L_B1); x.out[j][1] = x.out[j][2] = nullptr;
  }
}
// the operand copy of an activation [rows][cols] that no kernel wrote along with the fp32 tensor: bf16, or x3 pieces in PREC_X3
int operand_copy(const Plan& pl, Act a, int rows, int cols, hipStream_t st) {
  if (pl.prec == PREC_X3) return uniter_split3(a.f, rows, cols, cols, a.b, (size_t)3 * cols, (size_t)cols, st);
  return uniter_cast_bf16(a.f, a.b, (size_t)rows * cols, st);
}
// the keep flags drawn ahead for layer l's hidden-dropout site (second = 1: behind the FFN), NULL = the row pass draws them
static const unsigned char* hid_keep_bits(const Plan& pl, int l, int second) {
  return pl.hid_on ? pl.hid_keepb + (size_t)(2 * l + second) * pl.hid_stride : nullptr;
}
// Dropout + residual + LayerNorm behind layer l's attention output (second = 0) or FFN output (second = 1): t is `pieces` k-piece slabs
// of the product in front [M][H] each (one slab: stride 0, as uniter_ln_fwd_b16 passes it); y.b takes the operand copy of the result where the plan has one.  mean / rstd are kept
// only by a pass that saves for a backward pass.
// rows > 0: a pass over that many compacted rows, row r standing for row r * row_step of the plan's M (its dropout draw; head rows only)
int ln_fwd(uniter_model* m, hipStream_t st, int l, int second, const float* t, int pieces, const float* resid, float* z,
           Act y, float* mean, float* rstd, float ph, int rows = 0, int row_step = 1) {
  const Plan& pl = m->plan;
  const bool save = pl.mode != 0;
  const int M = rows > 0 ? rows : pl.M;
  const int g = second ? L_LN2_G : L_LN1_G;      // (its bias follows it)
  const int H = m->cfg.hidden_size;
  ProfScope ps(m, UNITER_K_LN, st);
  LnCall c;
  c.x = t; c.nslab = pieces; c.slab_stride = pieces > 1 ? (size_t)M * H : 0; c.res = resid; c.gamma = m->LP(l, g); c.beta = m->LP(l, g + 1);
  c.z = z; c.out = y.f; c.copy = y.b; c.pieces = pl.prec == PREC_X3 ? 3 : 1; c.M = M; c.H = H; c.stream = st;
  c.drop_row_step = row_step;
  if (save) { c.mean = mean; c.rstd = rstd; }
  c.drop = {ph, m->seed, m->offset, second ? SITE_FFN_OUT(l) : SITE_ATTN_OUT(l), hid_keep_bits(pl, l, second)};
  return ln_fwd_run(c);
}
// its backward row pass: dy is `pieces` slabs [M][H]; g takes the dropped gradient (fp32 and / or operand copy), ws the column partials
int ln_bwd(uniter_model* m, hipStream_t st, int l, int second, const float* dy, int pieces, const float* z, const float* mean,
           const float* rstd, float* dz, Act g, void* ws, float ph, int rows = 0, int row_step = 1) {
  const Plan& pl = m->plan;
  const int H = m->cfg.hidden_size;
  const int M = rows > 0 ? rows : pl.M;
  ProfScope ps(m, UNITER_K_LN_BWD, st);
  LnCall c;
  c.x = dy; c.nslab = pieces; c.slab_stride = (size_t)M * H; c.gamma = m->LP(l, second ? L_LN2_G : L_LN1_G);
  c.z = const_cast<float*>(z); c.mean = const_cast<float*>(mean); c.rstd = const_cast<float*>(rstd);      // (read only)
  c.dz = dz; c.out = g.f; c.copy = g.b; c.pieces = pl.prec == PREC_X3 ? 3 : 1; c.want_dbias = 1;
  c.M = M; c.H = H; c.ws = ws; c.ws_bytes = rows > 0 ? uniter_ln_bwd_ws_bytes(M, H) : pl.ln_ws_bytes; c.stream = st;
  c.drop_row_step = row_step;
  c.drop = {ph, m->seed, m->offset, second ? SITE_FFN_OUT(l) : SITE_ATTN_OUT(l), hid_keep_bits(pl, l, second)};      // (the forward pass's flags)
  return ln_bwd_rows_run(c);
}
// What the embeddings' forward and backward passes of the plan's batch state alike: ids, tables, LayerNorm weights, dims and the
// dropout identity (ph: the pass's hidden-dropout p).  The caller adds its outputs or gradients, workspace and stream.
static TxtEmbedCall txt_embed_call(const uniter_model* m, const uniter_batch_t& b, float ph) {
  const uniter_config_t& c = m->cfg;
  TxtEmbedCall e;
  e.ids = b.input_ids; e.pos_ids = b.position_ids; e.type_ids = b.txt_type_ids; e.word = m->P(P_WORD); e.pos = m->P(P_POS);
  e.type = m->P(P_TYPE); e.gamma = m->P(P_ELN_G); e.delta = m->ig.txt_delta;
  e.B = m->plan.B; e.T = m->plan.T; e.S = m->plan.S; e.H = c.hidden_size; e.vocab = c.vocab_size; e.max_pos = c.max_position_embeddings;
  e.type_vocab = c.type_vocab_size; e.pos_bcast = b.pos_bcast;
  e.drop = {ph, m->seed, m->offset, SITE_TXT_EMB};
  return e;
}
static ImgEmbedCall img_embed_call(const uniter_model* m, const uniter_batch_t& b, float ph) {
  const Plan& pl = m->plan;
  ImgEmbedCall e;
  e.imgfc = pl.imgfc; e.pos7 = b.img_pos_feat; e.type_ids = b.img_type_ids; e.Wp = m->P(P_POSL_W); e.bp = m->P(P_POSL_B);
  e.type = m->P(P_TYPE); e.g_i = m->P(P_ILN_G); e.b_i = m->P(P_ILN_B); e.g_p = m->P(P_PLN_G); e.b_p = m->P(P_PLN_B); e.g_f = m->P(P_FLN_G);
  e.B = pl.B; e.R = pl.R; e.T0 = pl.T0; e.S = pl.S; e.H = m->cfg.hidden_size; e.type_vocab = m->cfg.type_vocab_size;
  e.drop = {ph, m->seed, m->offset, SITE_IMG_EMB};
  return e;
}
// The four weight gradients of a layer in PREC_BF16 / PREC_X3, dW[p] [Mo[p], No[p]] += A[p]^T B[p] over the plan's M rows, in the grouped
// launch's order {W1, W2, QKV, attention output}.  Product 0 must be dW1 = dU^T y1: its A operand's column sums are intermediate.dense's
// bias gradient
// K[p]: product p's reduction length -- the plan's M, or B for the products of a last layer that ran on its head rows
struct WgradProducts { int Mo[4], No[4]; const void *A[4], *B[4]; float* dW[4]; int K[4]; };
// product p alone in PREC_BF16 (both operands k-major): split-K slabs + one reduce pass where that beats stream-K atomics into the
// gradient buffer (gemm_bf16.hip)
int wgrad_b16(uniter_model* m, const Plan& pl, hipStream_t st, const WgradProducts& t, int p) {
  const int Mo = t.Mo[p], No = t.No[p], K = pl.M;
  if (m->wg_overwrite) UCHECK_HIP(hipMemsetAsync(t.dW[p], 0, (size_t)Mo * No * sizeof(float), st));      // these forms accumulate
  const int pieces = gemm_bf16v2_wgrad_pieces(Mo, No, K);
  {
    ProfScope ps(m, UNITER_K_GEMM_WGRAD, st);
    const LaunchOpts lo = {ps.stamp, 0, m->launch_reserve};
    GemmCall c;
    c.M = Mo; c.N = No; c.K = K; c.A = {t.A[p], Mo, 0, 1}; c.B = {t.B[p], No, 0, 1}; c.ldc = No; c.stream = st;
    if (pieces == 0 || !pl.wg_slabs) {
      c.C = t.dW[p]; c.beta = 1; c.no_sk = pl.det ? 1 : 0;      // (deterministic plan: whole tiles, no stream-K)
      return gemm_bf16res_run(0, c, lo);
    }
    c.C = pl.wg_slabs; c.nsplit = pieces; c.c_split_stride = (long)Mo * No;
    UCHECK_RC(gemm_bf16v2_run(0, c, lo));
  }
  return uniter_slab_reduce_add(pl.wg_slabs, pieces, (size_t)Mo * No, t.dW[p], (size_t)Mo * No, st);
}
// bytes of LayerBufs::du_csum (make_plan): one row of I partial sums per 32 rows
inline size_t du_csum_bytes(int M, int I) { return (size_t)((M + 31) / 32) * I * sizeof(float); }
// Products idx[0 .. n) as ONE launch of whole-K tiles on the weight-gradient stream (gemm_bf16v2_wgrad_group / gemm_x3_wgrad_group by
// precision); colsum_after: followed by the column sums of dU (product 0's A operand), which nothing riding on the launch has taken
int wgrad_launch(uniter_model* m, int l, hipStream_t sd, const WgradProducts& t, const int* idx, int n, int cfg, int max_wgs,
                 uniter_x3_riders_t* riders, bool colsum_after) {
  const Plan& pl = m->plan;
  const bool x3 = pl.prec == PREC_X3;
  int Mo[4], No[4], Kp[4];
  const void *A[4], *B[4];
  float* dW[4];
  bool own_k = false;      // some product's reduction length is not the plan's M
  for (int i = 0; i < n; ++i) {
    Mo[i] = t.Mo[idx[i]]; No[i] = t.No[idx[i]]; A[i] = t.A[idx[i]]; B[i] = t.B[idx[i]]; dW[i] = t.dW[idx[i]]; Kp[i] = t.K[idx[i]];
    own_k = own_k || Kp[i] != pl.M;
  }
  WgradGroupCall c;
  c.n = n; c.Mo = Mo; c.No = No; c.K = pl.M; c.Kp = own_k ? Kp : nullptr; c.A = A; c.B = B; c.dW = dW; c.overwrite = m->wg_overwrite ? 1 : 0; c.max_wgs = max_wgs;
  c.riders = riders; c.stream = sd;
  {
    ProfScope ps(m, UNITER_K_GEMM_WGRAD, sd);
    const LaunchOpts lo = {ps.stamp, 0, m->launch_reserve};
    if (x3) {
      c.sk_ws = own_k ? nullptr : pl.sk_side; c.sk_ws_bytes = c.sk_ws ? pl.sk_bytes : 0;
      UCHECK_RC(gemm_x3_wgrad_group(cfg, c, lo));
    } else UCHECK_RC(gemm_bf16v2_wgrad_group(cfg, c, lo));
  }
  if (!colsum_after) return 0;
  const int rows = t.K[0];      // dU's rows (B behind a last layer on its head rows, whose dU column-partial buffer is the compact one)
  if (pl.det) {      // in a fixed order; the block partials go to the layer's dU column-partial buffer, which nothing else uses without riders
    const LayerBufs& lb = rows != pl.M ? pl.hr : pl.layers[l];
    return (x3 ? uniter_colsum_x3_add_det : uniter_colsum_bf16_add_det)(t.A[0], rows, t.Mo[0], t.Mo[0], m->LG(l, L_B1), lb.du_csum,
                                                                       du_csum_bytes(rows, t.Mo[0]), sd);
  }
  return (x3 ? uniter_colsum_x3_add : uniter_colsum_bf16_add)(t.A[0], rows, t.Mo[0], t.Mo[0], m->LG(l, L_B1), sd);      // intermediate.dense bias gradient
}

// Head rows only: rows b * L of a [B * L][cols] matrix into a compact [B][cols] one (gather), or back into their places (scatter);
// row_bytes = one row's bytes
int head_rows_gather(void* dst, const void* src, int B, int L, size_t row_bytes, hipStream_t st) {
  UCHECK_HIP(hipMemcpy2DAsync(dst, row_bytes, src, (size_t)L * row_bytes, row_bytes, (size_t)B, hipMemcpyDeviceToDevice, st));
  return 0;
}
int head_rows_scatter(void* dst, const void* src, int B, int L, size_t row_bytes, hipStream_t st) {
  UCHECK_HIP(hipMemcpy2DAsync(dst, (size_t)L * row_bytes, src, row_bytes, row_bytes, (size_t)B, hipMemcpyDeviceToDevice, st));
  return 0;
}
// The last layer's forward pass behind its attention kernel on the head rows (Plan::head_rows): the products with M = B and k-pieces
// of their own (Plan::hr_ns_h / hr_ns_i; the plan's other slab counts were picked for M = B * L), the row passes drawing row b * L's dropout, the B result rows into a
// zero-filled hidden_out.  x: the layer's input.
int head_rows_forward(uniter_model* m, hipStream_t st, int l, Act x, float* hidden_out, float ph) {
  Plan& pl = m->plan;
  const int H = m->cfg.hidden_size, I = m->cfg.intermediate_size, B = pl.B, L = pl.L;
  const LayerBufs& lb = pl.layers[l];
  LayerBufs& h = pl.hr;
  const bool save = pl.mode != 0;
  const size_t rowb = (size_t)H * sizeof(float);
  UCHECK_RC(head_rows_gather(h.ctx, lb.ctx, B, L, rowb, st));
  UCHECK_RC(head_rows_gather(pl.hr_x, x.f, B, L, rowb, st));
  const Act ctx = {h.ctx, h.ctxb}, y1 = {h.y1, h.y1b}, hact = {h.hact, h.hactb};
  UCHECK_RC(operand_copy(pl, ctx, B, H, st));
  UCHECK_RC(linear(m, UNITER_K_GEMM_ATTN_OUT_FWD, st, 0, B, H, H, l, L_OW, ctx, Act{h.t1, nullptr}, pl.hr_ns_h, UNITER_EPI_BIAS, m->LP(l, L_OB), nullptr,
                   nullptr));
  UCHECK_RC(ln_fwd(m, st, l, 0, h.t1, pl.hr_ns_h, pl.hr_x, h.z1, y1, h.mean1, h.rstd1, ph, B, L));
  float* gelu_aux = save ? h.u : h.hact;      // (as in the full pass: a pass that saves nothing parks gelu'(u) in the unused fp32 buffer)
  UCHECK_RC(linear(m, UNITER_K_GEMM_FFN_UP_FWD, st, 0, B, I, H, l, L_W1, y1, hact, 1, UNITER_EPI_BIAS_GELU_D, m->LP(l, L_B1), nullptr, gelu_aux));
  UCHECK_RC(linear(m, UNITER_K_GEMM_FFN_DOWN_FWD, st, 0, B, H, I, l, L_W2, hact, Act{h.t2, nullptr}, pl.hr_ns_i, UNITER_EPI_BIAS, m->LP(l, L_B2), nullptr,
                   nullptr));
  UCHECK_RC(ln_fwd(m, st, l, 1, h.t2, pl.hr_ns_i, h.y1, h.z2, Act{h.y2, nullptr}, h.mean2, h.rstd2, ph, B, L));
  // every other row of the output: exact zeros (a caller's hook never sees uninitialised rows)
  UCHECK_HIP(hipMemsetAsync(hidden_out, 0, (size_t)B * L * rowb, st));
  return head_rows_scatter(hidden_out, h.y2, B, L, rowb, st);
}

int validate_batch(const uniter_model* m, const uniter_batch_t* b) {
  UCHECK_ARG(b, "batch is NULL");
  UCHECK_ARG(b->B > 0 && b->L > 0, "batch: B and L must be positive");
  UCHECK_ARG(b->input_ids || b->img_feat, "batch: need input_ids and/or img_feat");
  UCHECK_ARG(b->attention_mask, "batch: attention_mask is NULL");
  if (b->input_ids) UCHECK_ARG(b->position_ids && b->T > 0, "batch: text needs position_ids and T > 0");
  if (b->img_feat) UCHECK_ARG(b->img_pos_feat && b->R > 0, "batch: image needs img_pos_feat and R > 0");
  const int S = (b->input_ids ? b->T : 0) + (b->img_feat ? b->R : 0);
  if (!(b->input_ids && b->img_feat && b->gather_index))
    UCHECK_SHAPE(b->L == S || (b->input_ids && b->img_feat && b->L <= S),
                 "batch: without gather_index L (%d) must equal T+R (%d)", b->L, S);
  UCHECK_SHAPE(b->T <= m->cfg.max_position_embeddings || !b->input_ids, "batch: T exceeds max_position_embeddings");
  return 0;
}

}  // namespace

// ------------------------------------------------------------------ C ABI ---
extern "C" int uniter_num_params(const uniter_config_t* cfg) {
  if (!cfg) return 0;
  return P_LAYER0 + cfg->num_hidden_layers * L_COUNT + 2;
}

extern "C" const char* uniter_param_name(const uniter_config_t* cfg, int i) {
  static thread_local char buf[128];
  if (!cfg || i < 0 || i >= uniter_num_params(cfg)) return nullptr;
  if (i < P_LAYER0) return kEmbNames[i];
  const int nl = cfg->num_hidden_layers;
  if (i < P_LAYER0 + nl * L_COUNT) {
    const int l = (i - P_LAYER0) / L_COUNT, k = (i - P_LAYER0) % L_COUNT;
    snprintf(buf, sizeof(buf), "encoder.layer.%d.%s", l, kLayerNames[k]);
    return buf;
  }
  return i == P_LAYER0 + nl * L_COUNT ? "pooler.dense.weight" : "pooler.dense.bias";
}

extern "C" int uniter_param_shape(const uniter_config_t* c, int i, int64_t* rows, int64_t* cols) {
  if (!c || !rows || !cols || i < 0 || i >= uniter_num_params(c)) return UNITER_E_ARG;
  const int64_t H = c->hidden_size, I = c->intermediate_size, D = c->img_dim;
  int64_t r = H, cc = 0;   // cols == 0 -> 1-D of length rows
  if (i < P_LAYER0) {
    switch (i) {
      case P_WORD: r = c->vocab_size; cc = H; break;
      case P_POS: r = c->max_position_embeddings; cc = H; break;
      case P_TYPE: r = c->type_vocab_size; cc = H; break;
      case P_IMG_W: r = H; cc = D; break;
      case P_POSL_W: r = H; cc = 7; break;
      case P_MASK_EMB: r = 2; cc = D; break;
      default: break;
    }
  } else if (i < P_LAYER0 + c->num_hidden_layers * L_COUNT) {
    switch ((i - P_LAYER0) % L_COUNT) {
      case L_QW: case L_KW: case L_VW: case L_OW: cc = H; break;
      case L_W1: r = I; cc = H; break;
      case L_B1: r = I; break;
      case L_W2: r = H; cc = I; break;
      default: break;
    }
  } else if (i == P_LAYER0 + c->num_hidden_layers * L_COUNT) {
    cc = H;
  }
  *rows = r; *cols = cc;
  return 0;
}

extern "C" int uniter_model_create(const uniter_config_t* cfg, float* const* params, float* const* grads,
                                   int n_params, uniter_model_t** out) {
  UCHECK_RC(check_cfg(cfg));
  UCHECK_ARG(params && out, "model_create: null pointer");
  UCHECK_ARG(n_params == uniter_num_params(cfg), "model_create: expected %d parameters, got %d",
             uniter_num_params(cfg), n_params);
  uniter_model* m = new uniter_model();
  m->cfg = *cfg;
  m->n_params = n_params;
  m->p.assign(params, params + n_params);
  if (grads) m->g.assign(grads, grads + n_params); else m->g.assign(n_params, nullptr);
  const size_t H = cfg->hidden_size;
  for (int i = 0; i < n_params; ++i) {
    if (!m->p[i] || ((uintptr_t)m->p[i] & 15)) {
      uniter_set_error("model_create: parameter %d (%s) is NULL or not 16-byte aligned", i, uniter_param_name(cfg, i));
      delete m; return UNITER_E_ARG;
    }
  }
  for (int l = 0; l < cfg->num_hidden_layers; ++l) {
    const bool ok = m->LP(l, L_KW) == m->LP(l, L_QW) + H * H && m->LP(l, L_VW) == m->LP(l, L_QW) + 2 * H * H &&
                    m->LP(l, L_KB) == m->LP(l, L_QB) + H && m->LP(l, L_VB) == m->LP(l, L_QB) + 2 * H;
    const bool gok = !grads || (m->LG(l, L_KW) == m->LG(l, L_QW) + H * H && m->LG(l, L_VW) == m->LG(l, L_QW) + 2 * H * H &&
                                m->LG(l, L_KB) == m->LG(l, L_QB) + H && m->LG(l, L_VB) == m->LG(l, L_QB) + 2 * H);
    if (!ok || !gok) {
      uniter_set_error("model_create: layer %d query/key/value weights (and biases, and their grads) must be contiguous", l);
      delete m; return UNITER_E_ARG;
    }
  }
  const int nl = cfg->num_hidden_layers;
  m->ev_main.resize(nl + 1); m->ev_side.resize(nl + 1); m->ev_mid.resize(nl + 1);
  for (int i = 0; i <= nl; ++i) {
    hipError_t e1 = hipEventCreateWithFlags(&m->ev_main[i], hipEventDisableTiming);
    if (e1 == hipSuccess) e1 = hipEventCreateWithFlags(&m->ev_mid[i], hipEventDisableTiming);
    hipError_t e2 = hipEventCreateWithFlags(&m->ev_side[i], hipEventDisableTiming);
    if (e1 != hipSuccess || e2 != hipSuccess) {
      uniter_set_error("model_create: hipEventCreate failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
      delete m; return (int)(e1 != hipSuccess ? e1 : e2);
    }
  }
  *out = m;
  return 0;
}

extern "C" void uniter_model_destroy(uniter_model_t* m) {
  if (!m) return;
  for (auto e : m->ev_main) if (e) hipEventDestroy(e);
  for (auto e : m->ev_side) if (e) hipEventDestroy(e);
  for (auto e : m->ev_mid) if (e) hipEventDestroy(e);
  for (auto e : m->prof_ev) if (e) hipEventDestroy(e);
  if (m->stamp_buf) (void)hipFree(m->stamp_buf);
  if (m->ev_aux0) hipEventDestroy(m->ev_aux0);
  if (m->ev_aux1) hipEventDestroy(m->ev_aux1);
  if (m->ev_aux2) hipEventDestroy(m->ev_aux2);
  if (m->ev_emb0) hipEventDestroy(m->ev_emb0);
  if (m->ev_emb1) hipEventDestroy(m->ev_emb1);
  if (m->ev_emb2) hipEventDestroy(m->ev_emb2);
  delete m;
}

extern "C" size_t uniter_model_ws_bytes(const uniter_model_t* m, int B, int T, int R, int L, int train) {
  if (!m) return 0;
  Plan pl;
  // sizes do not depend on pointers: carve from address 0; assume both modalities + masks (upper bound)
  make_plan(m, pl, nullptr, B, T > 0 ? T : 0, R > 0 ? R : 0, L, T > 0, R > 0, true, train);
  return pl.total + 256;
}

extern "C" int uniter_model_forward(uniter_model_t* m, const uniter_batch_t* b, float* hidden_out,
                                    int all_layers, int train, uint64_t seed, uint32_t offset, void* ws,
                                    size_t ws_bytes, void* stream) {
  uniter_model::AttnProbs ap;      // uniter_model_set_attn_probs: this pass's, forgotten whatever becomes of the pass
  bool head_rows_req = false;      // uniter_model_set_head_rows: this pass's, likewise
  if (m) { ap = m->ap_next; m->ap_next = uniter_model::AttnProbs(); head_rows_req = m->head_rows_next; m->head_rows_next = false; }
  UCHECK_ARG(m && hidden_out && ws, "model_forward: null pointer");
  m->launch_reserve = 0;      // (no collective of this step is in flight during its forward pass: the reserve is the backward pass's)
  UCHECK_ARG(train >= 0 && train <= 2, "model_forward: train must be 0, 1 or 2");
  UCHECK_RC(validate_batch(m, b));
  UCHECK_ARG(((uintptr_t)ws & 255) == 0, "model_forward: workspace must be 256-byte aligned");
  const uniter_config_t& c = m->cfg;
  const int H = c.hidden_size, I = c.intermediate_size, nl = c.num_hidden_layers, nh = c.num_attention_heads;
  const bool has_txt = b->input_ids != nullptr, has_img = b->img_feat != nullptr;
  Plan& pl = m->plan;
  const bool packed = b->cu_seqlens != nullptr;
  if (packed) {
    UCHECK_ARG(b->pack_src && b->pack_dst, "model_forward: packed mode needs pack_src and pack_dst");
    UCHECK_SHAPE(b->Mp > 0 && (int64_t)b->Mp <= (int64_t)b->B * b->L, "model_forward: bad Mp %d", b->Mp);
    UCHECK_SHAPE(b->L <= uniter_attn_varlen_max_len(), "model_forward: packed mode supports L <= %d (got %d)",
                 uniter_attn_varlen_max_len(), b->L);
  }
  const uniter_model::InputGrads ig = m->ig_next;      // uniter_model_set_input_grads: this pass's, whatever becomes of it
  m->ig_next = m->ig = uniter_model::InputGrads();
  if (ig.txt_delta || ig.outputs()) {
    UCHECK_ARG(has_txt || !(ig.txt_delta || ig.d_txt_rows), "model_forward: txt_delta / d_txt_rows set (uniter_model_set_input_grads) on a batch without text");
    UCHECK_ARG(has_img || !(ig.d_img_feat || ig.d_img_pos_feat), "model_forward: d_img_feat / d_img_pos_feat set (uniter_model_set_input_grads) on a batch without regions");
    UCHECK_ARG(train != 0 || !ig.outputs(), "model_forward: input gradients set (uniter_model_set_input_grads) for an inference forward (train = 0)");
    UCHECK_ARG((((uintptr_t)ig.txt_delta | (uintptr_t)ig.d_txt_rows | (uintptr_t)ig.d_img_feat) & 15) == 0,
               "model_forward: txt_delta, d_txt_rows and d_img_feat must be 16-byte aligned");
    UCHECK_SHAPE(!(ig.txt_delta || ig.d_txt_rows || ig.d_img_pos_feat) || (c.hidden_size % 4 == 0 && c.hidden_size <= 1024),
                 "model_forward: input gradients need hidden_size %% 4 == 0 and <= 1024 (got %d)", c.hidden_size);
    m->ig = ig;
  }
  const uniter_model::AttnGrads ag = m->ag_next;       // uniter_model_set_attn_grads: this pass's, whatever becomes of it
  m->ag_next = m->ag = uniter_model::AttnGrads();
  if (ag.out) {
    UCHECK_ARG(train != 0, "model_forward: attention gradients set (uniter_model_set_attn_grads) for an inference forward (train = 0)");
    UCHECK_ARG(train != 1 || !(c.attention_probs_dropout_prob > 0.f),
               "model_forward: attention gradients set (uniter_model_set_attn_grads) for a training forward with attention dropout: "
               "they are defined on the undropped probabilities");
    m->ag = ag;
  }
  make_plan(m, pl, ws, b->B, b->T, b->R, b->L, has_txt, has_img, b->img_masks != nullptr, train,
            packed ? b->Mp : -1);
  if (pl.total > ws_bytes) {
    uniter_set_error("model_forward: workspace too small (%zu < %zu)", ws_bytes, pl.total);
    return UNITER_E_WS;
  }
  hipStream_t st = (hipStream_t)stream;
  const float ph = train == 1 ? c.hidden_dropout_prob : 0.f;
  const float pa = train == 1 ? c.attention_probs_dropout_prob : 0.f;
  const int B = b->B, R = b->R, L = b->L, S = pl.S, M = pl.M;
  const bool save = train != 0;
  const Switches& sw = uniter_switches();
  const bool gelu_d = sw.gelu_d || pl.prec == PREC_X3;      // UNITER_GELU_D=0: A/B switch (store the pre-activation, libm erf twice)
  pl.gelu_d = gelu_d;
  m->batch = *b; m->hidden_out = hidden_out; m->all_layers = all_layers; m->seed = seed; m->offset = offset;
  m->bwd_open = false;
  ++m->generation;

  // the flag words of the balanced walk's two workspaces (16 KB each): zero before the first launch that uses them -- the launches
  // leave them zero, but the workspace is the caller's and may be a new one
  if (pl.sk_main) UCHECK_HIP(hipMemsetAsync(pl.sk_main, 0, 16384, st));
  if (pl.sk_side) UCHECK_HIP(hipMemsetAsync(pl.sk_side, 0, 16384, st));

  // dropout keep flags of the attention probabilities of ALL layers, drawn in one elementwise launch ahead of everything --
  // a function of (seed, offset) alone, so it runs while the optimizer still streams the word table the text branch waits for
  // (the L <= 192 kernels then read them; the backward pass reads the same words)
  bool keep_on_aux = false;
  bool keep_pre = sw.keep_pregen && save && pa > 0.f && L <= uniter_attn_varlen_max_len();
  if (keep_pre) {
    const size_t stride = nl > 1 ? (size_t)((char*)pl.layers[1].keepb - (char*)pl.layers[0].keepb) : 0;
    for (int l = 1; l < nl && keep_pre; ++l)
      keep_pre = (size_t)((char*)pl.layers[l].keepb - (char*)pl.layers[0].keepb) == stride * l;
    if (keep_pre) {
      // round 5: on the auxiliary stream when the caller gave one (uniter_model_set_aux_stream) -- 60 us of Philox rounds that
      // depend on (seed, offset) alone, beside the head of the forward pass (region projection, embeddings: small launches that
      // leave the chip empty) instead of in front of it; layer 0's attention waits for the event
      hipStream_t ks = st;
      if (m->aux && m->aux != st) {
        if (!m->ev_aux0) UCHECK_HIP(hipEventCreateWithFlags(&m->ev_aux0, hipEventDisableTiming));
        if (!m->ev_aux1) UCHECK_HIP(hipEventCreateWithFlags(&m->ev_aux1, hipEventDisableTiming));
        UCHECK_HIP(hipEventRecord(m->ev_aux0, st));            // the flags' last readers (the previous backward pass) ran on `st`
        UCHECK_HIP(hipStreamWaitEvent(m->aux, m->ev_aux0, 0));
        ks = m->aux;
      }
      UCHECK_RC(uniter_attn_keep_bits_gen(pl.layers[0].keepb, stride, nl, B, L, nh, pa, seed, offset, SITE_ATTN_PROBS(0),
                                          SITE_ATTN_PROBS(1) - SITE_ATTN_PROBS(0), ks));
      if (ks != st) { UCHECK_HIP(hipEventRecord(m->ev_aux1, ks)); keep_on_aux = true; }
    }
  }
  // the attention kernels of this plan, forward and backward: decided here, once, and only read from now on
  pl.attn_fwd = attn_kernel(pl, pa, save, keep_pre, false);
  pl.attn_bwd = attn_kernel(pl, pa, save, keep_pre, true);
  const bool attn_b16 = attn_is_b16(pl.attn_fwd);
  // the hidden dropout's keep flags (the two dropout + residual + LayerNorm passes of every layer, forward AND backward) behind them
  // on the same stream: OFF by default (UNITER_HIDDEN_PREGEN=1 switches it on)
  pl.hid_on = false;
  if (sw.hidden_pregen && save && ph > 0.f && m->aux && m->aux != st && pl.hid_keepb) {
    if (!m->ev_aux0) UCHECK_HIP(hipEventCreateWithFlags(&m->ev_aux0, hipEventDisableTiming));
    if (!m->ev_aux2) UCHECK_HIP(hipEventCreateWithFlags(&m->ev_aux2, hipEventDisableTiming));
    if (!keep_on_aux) {      // (no attention flags were drawn on the stream: order it behind the flags' last readers ourselves)
      UCHECK_HIP(hipEventRecord(m->ev_aux0, st));
      UCHECK_HIP(hipStreamWaitEvent(m->aux, m->ev_aux0, 0));
    }
    UCHECK_RC(uniter_hidden_keep_bits_gen(pl.hid_keepb, pl.hid_stride, 2 * nl, SITE_ATTN_OUT(0), SITE_FFN_OUT(0),
                                          SITE_ATTN_OUT(1) - SITE_ATTN_OUT(0), (size_t)M * H, ph, seed, offset, m->aux));
    UCHECK_HIP(hipEventRecord(m->ev_aux2, m->aux));
    pl.hid_on = true;
  }

  // Head rows only (uniter_model_set_head_rows): honoured where the plan carved the compact buffers (precision 3, padded batch) and the
  // pass has one output layer.  The schedule switches that are bit-neutral on the full path stay so here: keep flags of the hidden
  // dropout drawn ahead are addressed by the original row's group index (LnCall::drop_row_step), an attention-gradient capture reads
  // the zero-filled full-size gradient of the context, and the balanced walk's workspaces go to the products that can use them
  pl.head_rows = head_rows_req && pl.prec == PREC_X3 && !packed && pl.hr.ctx && !all_layers;

  // parameters still being written by an optimizer step on another stream (uniter_model_set_ready_events)
  // ready = [embeddings, layer 0 .. nl-1] or, with one more event, [embeddings WITHOUT the word table, layers.., word table]:
  // the image branch (region projection, 3 LayerNorms) then runs while the optimizer still streams the 89-MB word table
  const bool gated = (int)m->ready.size() == nl + 1 || (int)m->ready.size() == nl + 2;
  const bool word_split = (int)m->ready.size() == nl + 2;
  if (gated) UCHECK_HIP(hipStreamWaitEvent(st, m->ready[0], 0));

  // ---- embeddings (model/model.py:321-334) ----
  if (has_img) {
    const float* feat = b->img_feat;
    if (b->img_masks) {
      UCHECK_RC(uniter_img_mask_add(b->img_feat, b->img_masks, m->P(P_MASK_EMB), pl.feat_eff, B * R, c.img_dim, st));
      feat = pl.feat_eff;
    }
    // region-feature projection (model/model.py:267): 576 x 768 outputs are 108 tiles of 64 x 64 for 1024 workgroup slots
    // with K = 2048 -- as a stream-K accumulation on top of the bias rows it fills the chip (fp32: 58 -> 25 us)
    const long t64 = (long)((B * R + 63) / 64) * ((H + 63) / 64);
    // (UNITER_IMG_SK; native fp32 only: the float atomics make the sum's order vary from run to run, switches.h)
    // (nor with uniter_model_set_deterministic on: the bias-epilogue form whatever the switch says)
    if (sw.img_sk && !m->deterministic && pl.prec == PREC_F32 && t64 >= 8 && t64 <= 600 && c.img_dim >= 1024 && c.img_dim % 64 == 0 && H % 4 == 0) {
      UCHECK_RC(uniter_bias_rows(m->P(P_IMG_B), pl.imgfc, B * R, H, st));
      UCHECK_RC(gemm(m, 0, st, 0, 0, B * R, H, c.img_dim, feat, c.img_dim, m->P(P_IMG_W), c.img_dim, pl.imgfc, H,
                     UNITER_EPI_NONE, nullptr, nullptr, nullptr, 0, 1));
    } else {
      UCHECK_RC(gemm(m, 0, st, 0, 0, B * R, H, c.img_dim, feat, c.img_dim, m->P(P_IMG_W), c.img_dim, pl.imgfc, H,
                     UNITER_EPI_BIAS, m->P(P_IMG_B), nullptr, nullptr, 0, 0));
    }
    ImgEmbedCall e = img_embed_call(m, *b, ph);
    e.b_f = m->P(P_FLN_B); e.cat = pl.cat; e.stats = save ? pl.img_stats : nullptr; e.stream = st;
    UCHECK_RC(img_embed_fwd_run(e));
  }
  if (has_txt) {
    if (word_split) UCHECK_HIP(hipStreamWaitEvent(st, m->ready[nl + 1], 0));
    TxtEmbedCall e = txt_embed_call(m, *b, ph);      // (with m->ig.txt_delta, the perturbation of the word rows, where one is set)
    e.beta = m->P(P_ELN_B); e.cat = pl.cat; e.stream = st;
    UCHECK_RC(txt_embed_fwd_run(e));
  }
  if (!save) m->ig = uniter_model::InputGrads();      // an inference forward: no backward pass follows
  const bool joint = has_txt && has_img;
  // (round 6) the joint rows and their operand copy for layer 0's first product in ONE launch: this chain -- text embeddings, gather,
  // split -- is what the first encoder product waits for behind the optimizer's update of the word table
  const bool fuse_copy = sw.gather_ex && !packed && pl.copies() && H <= 1024 && m->mirror != nullptr;
  if (packed) UCHECK_RC(uniter_row_gather(pl.cat, b->pack_src, pl.emb, M, H, B * S, st));
  else if (fuse_copy) UCHECK_RC(uniter_gather_rows_ex(pl.cat, joint ? b->gather_index : nullptr, pl.emb, pl.embb, pl.prec == PREC_X3 ? 1 : 2, B, S, L, H, st));
  else UCHECK_RC(uniter_gather_rows(pl.cat, joint ? b->gather_index : nullptr, pl.emb, B, S, L, H, st));
  const size_t PH = (size_t)B * L * H;          // one layer of the padded output
  Act x = {pl.emb, pl.embb};
  if (pl.copies() && !fuse_copy) {
    UCHECK_ARG(m->mirror != nullptr, "model_forward: precision 2 / 3 needs uniter_model_set_weight_mirror");
    UCHECK_RC(operand_copy(pl, x, M, H, st));
  }
  // ---- encoder (model/model.py:282-292; model/layer.py:166-170) ----
  const float* mask = packed ? nullptr : b->attention_mask;
  const int32_t* cu_seqlens = packed ? b->cu_seqlens : nullptr;
  // the context's operand copy is made after the fact where the attention kernel left none: PREC_BF16 unless the kernel was a bf16 one;
  // PREC_X3 beyond the L <= 192 kernels only
  const bool ctx_copy = pl.prec == PREC_BF16 ? !attn_b16 : pl.prec == PREC_X3 && L > uniter_attn_varlen_max_len();
  for (int l = 0; l < nl; ++l) {
    LayerBufs& lb = pl.layers[l];
    if (gated) UCHECK_HIP(hipStreamWaitEvent(st, m->ready[1 + l], 0));
    if (l == 0 && keep_on_aux) UCHECK_HIP(hipStreamWaitEvent(st, m->ev_aux1, 0));      // the keep flags of every layer are drawn
    float* y2 = packed ? lb.y2 : (all_layers ? hidden_out + l * PH : (l == nl - 1 ? hidden_out : lb.y2));
    // (the bf16 attention kernels read Q, K, V as bf16: the product writes only that, in the qkv buffer's place)
    const Act qkv = attn_b16 ? Act{nullptr, (unsigned short*)lb.qkv} : Act{lb.qkv, nullptr};
    UCHECK_RC(linear(m, UNITER_K_GEMM_QKV_FWD, st, 0, M, 3 * H, H, l, L_QW, x, qkv, 1, UNITER_EPI_BIAS, m->LP(l, L_QB), nullptr, nullptr));
    {
      ProfScope ps(m, UNITER_K_ATTN_FWD, st);
      const AttnKernel k = pl.attn_fwd;
      const bool flags_only = attn_reads_flags_only(k);
      AttnCall c;
      c.B = B; c.L = L; c.nh = nh; c.qkv = lb.qkv; c.qkv_is_bf16 = attn_b16; c.mask = mask; c.cu_seqlens = cu_seqlens;
      c.ctx = lb.ctx; c.lse = lb.lse; c.p_drop = pa; c.stream = st;
      // the context leaves the kernel in the operand format too (precision 2: bf16, 3: x3 pieces), but for the two plain fp32 forms
      c.ctx_copy = (k == ATTN_F32 || k == ATTN_F32_PRE) ? nullptr : lb.ctxb;
      c.pieces = pl.prec == PREC_X3 ? 3 : 1;
      // the dropout keep flags: attention_x3.hip's kernels only read them; the others draw them (or read them: keep_pre) and write
      // them for the backward pass of a plan that is saved -- never the any-length form
      c.keep_bits = (k != ATTN_F32 && (flags_only || save)) ? lb.keepb : nullptr;
      c.keep_ready = c.keep_bits && (flags_only || keep_pre);
      c.seed = flags_only ? 0 : seed; c.offset = flags_only ? 0 : offset; c.site = flags_only ? 0 : SITE_ATTN_PROBS(l);
      UCHECK_RC(attn_forward(k, "attn_forward", c));
    }
    // the probabilities as an output (uniter_model_set_attn_probs): here, because only between this layer's attention launch and the
    // next layer's query|key|value product does lb.qkv hold layer l's values in a pass that saves nothing
    if (ap.out)
      UCHECK_RC(uniter_attn_probs(lb.qkv, attn_b16 ? 1 : 0, mask, cu_seqlens, ap.out + (size_t)l * ap.stride, B, L, nh, ap.head_mean, st));
    // the context's operand copy: operand of the projection below and of its weight gradient
    if (pl.head_rows && l == nl - 1) {      // the rest of the last layer on the rows the caller reads
      UCHECK_RC(head_rows_forward(m, st, l, x, hidden_out, ph));
      break;
    }
    const Act ctx = {lb.ctx, lb.ctxb}, y1 = {lb.y1, lb.y1b}, hact = {lb.hact, lb.hactb};
    if (ctx_copy) UCHECK_RC(operand_copy(pl, ctx, M, H, st));
    UCHECK_RC(linear(m, UNITER_K_GEMM_ATTN_OUT_FWD, st, 0, M, H, H, l, L_OW, ctx, Act{lb.t1, nullptr}, pl.ns_kh, UNITER_EPI_BIAS,
                     m->LP(l, L_OB), nullptr, nullptr));
    if (l == 0 && pl.hid_on) UCHECK_HIP(hipStreamWaitEvent(st, m->ev_aux2, 0));      // every layer's hidden keep flags are drawn
    UCHECK_RC(ln_fwd(m, st, l, 0, lb.t1, pl.ns_kh, x.f, lb.z1, y1, lb.mean1, lb.rstd1, ph));
    // FFN-up writes gelu'(u) (or u: gelu_d) beside the activation, for the backward pass.  With operand copies the activation exists only
    // as one (operand of FFN-down and of its weight gradient), and a pass that saves nothing parks gelu'(u) in the unused fp32 buffer;
    // gelu'(u) is bf16 in PREC_BF16 and fp32 elsewhere (linear())
    float* gelu_aux = save ? lb.u : (pl.copies() ? lb.hact : nullptr);
    UCHECK_RC(linear(m, UNITER_K_GEMM_FFN_UP_FWD, st, 0, M, I, H, l, L_W1, y1, hact, 1, gelu_d ? UNITER_EPI_BIAS_GELU_D : UNITER_EPI_BIAS_GELU,
                     m->LP(l, L_B1), nullptr, gelu_aux));
    UCHECK_RC(linear(m, UNITER_K_GEMM_FFN_DOWN_FWD, st, 0, M, H, I, l, L_W2, hact, Act{lb.t2, nullptr}, pl.ns_ki, UNITER_EPI_BIAS,
                     m->LP(l, L_B2), nullptr, nullptr));
    UCHECK_RC(ln_fwd(m, st, l, 1, lb.t2, pl.ns_ki, lb.y1, lb.z2, Act{y2, lb.y2b}, lb.mean2, lb.rstd2, ph));
    lb.y2 = y2;
    x = Act{y2, lb.y2b};
    if (packed && (all_layers || l == nl - 1)) {
      // padded [B, L, H] view for the caller: valid rows scattered, padded positions zero
      float* dst = all_layers ? hidden_out + l * PH : hidden_out;
      UCHECK_HIP(hipMemsetAsync(dst, 0, PH * sizeof(float), st));
      UCHECK_RC(uniter_row_scatter_add(y2, b->pack_dst, dst, M, H, B * L, st));
    }
  }
  m->ready.clear();
  return 0;
}

extern "C" int uniter_model_backward_begin(uniter_model_t* m, const uniter_batch_t* b, const float* d_hidden,
                                           int all_layers, uint64_t seed, uint32_t offset, void* ws,
                                           size_t ws_bytes, void* stream, void* side_stream) {
  UCHECK_ARG(m && d_hidden && ws, "backward_begin: null pointer");
  if (m->plan.mode == 0 || m->hidden_out == nullptr) {
    uniter_set_error("backward_begin: no training-mode forward precedes this call");
    return UNITER_E_STATE;
  }
  UCHECK_ARG(m->seed == seed && m->offset == offset && m->all_layers == all_layers,
             "backward_begin: seed/offset/all_layers differ from the forward call");
  for (int i = 0; i < m->n_params; ++i)
    UCHECK_ARG(m->g[i] != nullptr, "backward: gradient buffer %d (%s) is NULL", i, uniter_param_name(&m->cfg, i));
  (void)ws_bytes; (void)b;
  m->d_hidden = d_hidden;
  m->st = (hipStream_t)stream;
  m->side = side_stream ? (hipStream_t)side_stream : (hipStream_t)stream;
  m->bwd_open = true;
  return 0;
}

extern "C" int uniter_model_backward_layer(uniter_model_t* m, int l) {
  UCHECK_ARG(m, "backward_layer: null model");
  m->launch_reserve = m->cu_reserve;
  if (!m->bwd_open) { uniter_set_error("backward_layer: call uniter_model_backward_begin first"); return UNITER_E_STATE; }
  const uniter_config_t& c = m->cfg;
  const int H = c.hidden_size, I = c.intermediate_size, nl = c.num_hidden_layers, nh = c.num_attention_heads;
  UCHECK_ARG(l >= 0 && l < nl, "backward_layer: bad layer %d", l);
  Plan& pl = m->plan;
  const int B = pl.B, L = pl.L, M = pl.M;
  const float ph = pl.mode == 1 ? c.hidden_dropout_prob : 0.f;
  const float pa = pl.mode == 1 ? c.attention_probs_dropout_prob : 0.f;
  hipStream_t st = m->st, sd = m->side;
  LayerBufs& lb = pl.layers[l];
  const Act x = l == 0 ? Act{pl.emb, pl.embb} : Act{pl.layers[l - 1].y2, pl.layers[l - 1].y2b};      // the layer's input
  const size_t MH = (size_t)M * H;

  // upstream gradient w.r.t. this layer's output (packed mode: the caller's padded gradient gathered
  // to the valid rows; gradients at padded positions are dropped, as nothing was computed there)
  const float* dy;
  const float* dh = nullptr;
  if (l == nl - 1 || m->all_layers) {
    dh = m->d_hidden + (m->all_layers ? (size_t)l * ((size_t)B * L * H) : 0);
    if (pl.packed) {
      UCHECK_RC(uniter_row_gather(dh, m->batch.pack_dst, pl.dpk, M, H, B * L, st));
      dh = pl.dpk;
    }
  }
  // the last layer of a plan that ran on its head rows (Plan::head_rows): the stretch in front of the attention backward on pl.hr's
  // B rows -- pb, Mp rows, row r standing for row r * row_step; every other layer: the layer's own buffers, M rows
  const bool hr = pl.head_rows && l == nl - 1;
  LayerBufs& pb = hr ? pl.hr : lb;
  const int Mp = hr ? B : M, row_step = hr ? L : 1;
  if (hr) {
    UCHECK_RC(head_rows_gather(pl.hr_dy, dh, B, L, (size_t)H * sizeof(float), st));
    dy = pl.hr_dy;
  } else if (l == nl - 1) {
    dy = dh;
  } else if (m->all_layers) {
    UCHECK_RC(launch_add_f32(pl.dsum, pl.layers[l + 1].dx, dh, MH, st));
    dy = pl.dsum;
  } else {
    dy = pl.layers[l + 1].dx;
  }
  // the dropped gradient in fp32: the operand of the fp32 GEMMs; the bf16-resident GEMMs read its bf16 copy only, so
  // the fp32 store (8 MB per pass) is skipped there
  const bool copies = pl.copies();
  const Act g2 = {ph > 0.f ? (copies ? nullptr : pb.g2) : pb.dz2, pb.g2b};
  const Act g1 = {ph > 0.f ? (copies ? nullptr : pb.g1) : pb.dz1, pb.g1b};
  // precision 2: the next layer's dx may be split-K slabs (summed here); never for the last layer (dy is the caller's
  // gradient), with all_layers (dy is dsum) or in layer 0 (the embedding backward reads a plain dx)
  const int ns_dy = (l == nl - 1 || m->all_layers) ? 1 : pl.ns_k3h;
  const int ns_dx = (l == 0 || m->all_layers) ? 1 : pl.ns_k3h;
  UCHECK_RC(ln_bwd(m, st, l, 1, dy, ns_dy, pb.z2, pb.mean2, pb.rstd2, pb.dz2, g2, pb.ln_ws2, ph, hr ? Mp : 0, row_step));
  // FFN down dgrad (+ GELU'), FFN up dgrad (+ residual grad)
  // the GEMM's epilogue also emits per-32-row column sums of du (= partial bias gradients of
  // intermediate.dense): saves a 32 MB re-read of du
  const bool fuse_db1 = H % 64 == 0;
  const Switches& sw = uniter_switches();
  const bool attn_b16 = attn_is_b16(pl.attn_bwd);
  // the L <= 192 attention backward kernels (every one but uniter_attn_bwd) also emit the per-sample column sums of dqkv (the fused
  // query|key|value bias gradient before its sum over the batch): no 24 MB re-read of dqkv
  const bool fused_qb = pl.attn_bwd != ATTN_F32;
  // precision 3 with the x3 attention backward: the attention-output input gradient leaves as k-pieces (the kernel sums them)
  // (head rows: one slab -- it is placed into the zero-filled full-size buffer the attention backward reads)
  const int ns_dctx = hr ? 1 : (pl.attn_bwd == ATTN_X3 && sw.dctx_split) ? pl.ns_kh_b : 1;
  const int ns_dy1 = hr ? pl.hr_ns_i : pl.ns_ki_b;
  const int epi_du = pl.gelu_d ? UNITER_EPI_MUL : UNITER_EPI_DGELU;
  // what rides on the layer's grouped weight-gradient launch (precisions 2 and 3), and that launch's geometry
  const WgradGroup wg = copies ? wgrad_group(m, pl, l, m->launch_reserve, hr && Mp != M) : WgradGroup();
  // dU = (g2 . W2) * gelu'(u): with operand copies it exists only as one (operand of the next product and of intermediate.dense's weight
  // gradient).  Its column sums (that layer's bias gradient) start here as column partials: per 32 rows in the fp32 kernels; with operand
  // copies only when riders of the 128 x 256 weight-gradient geometry finish them (one row of partial sums per 64 rows of dU)
  const Act du = {pb.du, pb.dub}, dqkv = {lb.dqkv, lb.dqkvb};
  UCHECK_RC(linear(m, UNITER_K_GEMM_DGRAD, st, 1, Mp, I, H, l, L_W2, g2, du, 1, epi_du, nullptr, pb.u, nullptr,
                   (copies ? wg.colpart : fuse_db1) ? pb.du_csum : nullptr));
  UCHECK_RC(linear(m, UNITER_K_GEMM_DGRAD, st, 1, Mp, H, I, l, L_W1, du, Act{pb.dy1, nullptr}, ns_dy1, UNITER_EPI_ADD, nullptr, pb.dz2,
                   nullptr));
  UCHECK_RC(ln_bwd(m, st, l, 0, pb.dy1, ns_dy1, pb.z1, pb.mean1, pb.rstd1, pb.dz1, g1, pb.ln_ws1, ph, hr ? Mp : 0, row_step));
  // the layer's weight gradients in precisions 2 and 3 (WgradProducts): the query|key|value one always reduces over the plan's M rows
  const WgradProducts wp = {{I, H, 3 * H, H}, {H, I, H, H}, {pb.dub, pb.g2b, lb.dqkvb, pb.g1b}, {pb.y1b, pb.hactb, x.b, pb.ctxb},
                            {m->LG(l, L_W1), m->LG(l, L_W2), m->LG(l, L_QW), m->LG(l, L_OW)}, {Mp, Mp, M, Mp}};
  const int wp_all[4] = {0, 1, 2, 3}, wp_early[3] = {0, 1, 3}, wp_late[1] = {2};
  const bool wg_early = pl.prec == PREC_BF16 && pl.wg_group >= 2 && sd != st;
  if (wg_early) {
    // the three weight gradients whose operands exist now (FFN down / up, attention output: 324 whole-K tiles) start on
    // the side stream here, next to the attention backward (192 workgroups with large LDS: a quarter of the CUs idle)
    UCHECK_HIP(hipEventRecord(m->ev_mid[l], st));
    UCHECK_HIP(hipStreamWaitEvent(sd, m->ev_mid[l], 0));
    UCHECK_RC(wgrad_launch(m, l, sd, wp, wp_early, 3, 1, 0, nullptr, true));
  }
  // (two k-pieces when the x3 attention backward follows: it sums the slabs while it reads them -- 126 tiles do not fill the chip)
  UCHECK_RC(linear(m, UNITER_K_GEMM_DGRAD, st, 1, Mp, H, H, l, L_OW, g1, Act{pb.dctx, nullptr}, ns_dctx, UNITER_EPI_NONE, nullptr, nullptr,
                   nullptr));
  if (hr) {
    // what the attention backward and the QKV input gradient read over all M rows -- the context's gradient and the residual branch's
    // gradient lb.dz1 -- is zero outside the head rows: zero-fill, then the B rows into their places
    const size_t rowb = (size_t)H * sizeof(float);
    UCHECK_HIP(hipMemsetAsync(lb.dctx, 0, MH * sizeof(float), st));
    UCHECK_RC(head_rows_scatter(lb.dctx, pb.dctx, B, L, rowb, st));
    UCHECK_HIP(hipMemsetAsync(lb.dz1, 0, MH * sizeof(float), st));
    UCHECK_RC(head_rows_scatter(lb.dz1, pb.dz1, B, L, rowb, st));
  }
  // the gradient-weighted attention as an output (uniter_model_set_attn_grads): here, because only between the product that wrote
  // dctx and the attention backward that consumes it do this layer's qkv and dctx both hold what the pass computed
  if (m->ag.out) {
    const uniter_model::AttnGrads& ag = m->ag;
    UCHECK_RC(uniter_attn_grad(lb.qkv, attn_b16 ? 1 : 0, pl.packed ? nullptr : m->batch.attention_mask, pl.packed ? m->batch.cu_seqlens : nullptr,
                               lb.dctx, ns_dctx, MH, ag.out + (size_t)l * ag.stride,
                               ag.head_sums ? ag.head_sums + (size_t)l * B * nh : nullptr, ag.ws, ag.ws_bytes, B, L, nh, ag.reduce, st));
  }
  {
    ProfScope ps(m, UNITER_K_ATTN_BWD, st);
    const AttnKernel k = pl.attn_bwd;
    const bool flags_only = attn_reads_flags_only(k);
    AttnCall c;
    c.B = B; c.L = L; c.nh = nh; c.qkv = lb.qkv; c.qkv_is_bf16 = attn_b16;
    c.mask = pl.packed ? nullptr : m->batch.attention_mask; c.cu_seqlens = pl.packed ? m->batch.cu_seqlens : nullptr;
    c.ctx = lb.ctx; c.lse = lb.lse; c.p_drop = pa; c.stream = st;
    // the flags the forward pass of a saved plan left; without them the kernels that can draw repeat the forward pass's draw
    c.keep_bits = fused_qb ? lb.keepb : nullptr;
    c.seed = flags_only ? 0 : m->seed; c.offset = flags_only ? 0 : m->offset; c.site = flags_only ? 0 : SITE_ATTN_PROBS(l);
    c.dctx = lb.dctx; c.dctx_slabs = ns_dctx; c.dctx_slab_stride = ns_dctx > 1 ? MH : 0;
    // dqkv leaves the kernel in the operand format only (nothing reads an fp32 copy in those modes), but for the two plain fp32 forms
    const bool copy_out = k != ATTN_F32 && k != ATTN_F32_PRE;
    c.dqkv = copy_out ? nullptr : lb.dqkv; c.dqkv_copy = copy_out ? lb.dqkvb : nullptr; c.pieces = pl.prec == PREC_X3 ? 3 : 1;
    c.bias_part = fused_qb ? lb.qb_part : nullptr; c.delta = lb.delta;
    c.ws = flags_only ? nullptr : pl.attn_ws; c.ws_bytes = flags_only ? 0 : pl.attn_ws_bytes;
    c.det = pl.det;      // the kernel's bias partials in a fixed order
    UCHECK_RC(attn_backward(k, "attn_backward", c));
  }
  // dqkv's operand copy where the attention kernel left none: PREC_BF16 unless the kernel was a bf16 one; PREC_X3 behind uniter_attn_bwd only
  if (pl.prec == PREC_BF16 ? !attn_b16 : pl.prec == PREC_X3 && !fused_qb) UCHECK_RC(operand_copy(pl, dqkv, M, 3 * H, st));
  UCHECK_RC(linear(m, UNITER_K_GEMM_DGRAD, st, 1, M, H, 3 * H, l, L_QW, dqkv, Act{lb.dx, nullptr}, ns_dx, UNITER_EPI_ADD, nullptr, lb.dz1,
                   nullptr));

  // weight / bias gradients on the side stream (accumulate into the bound grad buffers)
  if (sd != st) {
    UCHECK_HIP(hipEventRecord(m->ev_main[l], st));
    UCHECK_HIP(hipStreamWaitEvent(sd, m->ev_main[l], 0));
  }
  // with riders (wgrad_group(): the default of precision 3) the column reductions below, the bias gradient of intermediate.dense and the
  // layer's share of the clip norm RIDE on the grouped weight-gradient launch -- no finalize / column-sum / sum-of-squares launches
  // on this stream
  // LayerNorm / dense-bias gradients: the column reductions of the two row passes above, the attention backward's
  // per-sample query|key|value bias partials and (fp32 mode) the dU column partials -- ONE launch for all of them
  if (!wg.riders) {
    const int lnp = ln_bwd_partial_rows(Mp);
    const float* parts[4] = {(const float*)pb.ln_ws2, (const float*)pb.ln_ws1, fused_qb ? lb.qb_part : nullptr,
                             (!copies && fuse_db1) ? pb.du_csum : nullptr};
    const int nparts[4] = {lnp, lnp, B, (Mp + 31) / 32};
    const size_t strides[4] = {(size_t)3 * H, (size_t)3 * H, (size_t)3 * H, (size_t)I};
    float* const outs[4][3] = {{m->LG(l, L_LN2_G), m->LG(l, L_LN2_B), m->LG(l, L_B2)},
                               {m->LG(l, L_LN1_G), m->LG(l, L_LN1_B), m->LG(l, L_OB)},
                               {m->LG(l, L_QB), nullptr, nullptr},
                               {m->LG(l, L_B1), nullptr, nullptr}};
    const int nout[4] = {3, 3, 1, 1};
    const int seg[4] = {H, H, 3 * H, I};
    UCHECK_RC(finalize_partials_jobs(4, PartialJobs{parts, nparts, strides, outs, nout, seg}, sd));
  }
  if (wg_early) {
    UCHECK_RC(wgrad_launch(m, l, sd, wp, wp_late, 1, 1, 0, nullptr, false));
  } else if (pl.prec == PREC_X3 || pl.wg_group) {
    // all four weight gradients of the layer as ONE launch of whole-K tiles, no atomics (432 tiles for UNITER-base: for 512 workgroup
    // slots in PREC_BF16; PREC_X3: persistent, wg.max_wgs caps its grid -- 0 = one workgroup per CU; layer 0: the smallest grid of as
    // many rounds)
    uniter_x3_riders_t riders;
    memset(&riders, 0, sizeof(riders));
    if (wg.riders) {
      if (m->norm_parts) {
        UCHECK_ARG((size_t)wg.slots <= m->norm_stride, "backward_layer: %d clip-norm slots per layer, room for %zu (uniter_model_set_norm_partials)",
                   wg.slots, m->norm_stride);
        riders.ssq = m->norm_parts + (size_t)l * m->norm_stride;
        // (a launch that left the balanced walk fills fewer slots than the layer's launch on the walk would: the rest read as zero)
        const int walk = (hr && pl.sk_side) ? wgrad_group(m, pl, l, m->launch_reserve).slots : wg.slots;
        if (walk > wg.slots && (size_t)walk <= m->norm_stride) UCHECK_HIP(hipMemsetAsync(riders.ssq + wg.slots, 0, (size_t)(walk - wg.slots) * sizeof(double), sd));
      }
      LayerBufs rb = pb;      // (the row passes' and dU's column partials: Mp rows' worth; the attention backward's bias partials: the layer's own)
      rb.qb_part = lb.qb_part;
      fill_layer_riders(riders, m, l, rb, Mp, B, H, fused_qb, wg.colpart);
    }
    UCHECK_RC(wgrad_launch(m, l, sd, wp, wp_all, 4, wg.cfg, wg.max_wgs, wg.riders ? &riders : nullptr, !wg.riders));
  } else if (pl.prec == PREC_BF16) {
    UCHECK_RC(wgrad_b16(m, pl, sd, wp, 1));
    UCHECK_RC(wgrad_b16(m, pl, sd, wp, 0));
    // intermediate.dense bias gradient (deterministic plan: in a fixed order, partials in the otherwise unused dU column-partial buffer)
    if (pl.det) UCHECK_RC(uniter_colsum_bf16_add_det(lb.dub, M, I, I, m->LG(l, L_B1), lb.du_csum, du_csum_bytes(M, I), sd));
    else UCHECK_RC(uniter_colsum_bf16_add(lb.dub, M, I, I, m->LG(l, L_B1), sd));
    UCHECK_RC(wgrad_b16(m, pl, sd, wp, 3));
    UCHECK_RC(wgrad_b16(m, pl, sd, wp, 2));
  } else {
    const int wb = m->wg_overwrite ? -1 : 1;      // -1: overwrite (or clear, then accumulate) -- see gemm()
    // the layer's four weight gradients as ONE persistent launch of whole-K tiles (uniter_wgrad_f32_group): layer 0 only by default
    // (UNITER_WGRAD_GROUP_F32 = 2; 0 = never, 1 = every layer: measured slower, switches.h), and only when every shape is on whole tiles
    const bool group_env = sw.wgrad_group_f32 == 1 || (sw.wgrad_group_f32 == 2 && l == 0);
    bool grouped = false;
    if (group_env && sw.wgrad_whole == 15 && sw.wgrad_cfg == 0 && pl.prec == PREC_F32 && fuse_db1) {
      const int Mo[4] = {H, I, H, 3 * H}, No[4] = {I, H, H, H};
      const void* const As[4] = {g2.f, lb.du, g1.f, lb.dqkv};
      const void* const Bs[4] = {lb.hact, lb.y1, lb.ctx, x.f};
      float* const dWs[4] = {m->LG(l, L_W2), m->LG(l, L_W1), m->LG(l, L_OW), m->LG(l, L_QW)};
      ProfScope ps(m, UNITER_K_GEMM_WGRAD, sd);
      WgradGroupCall c;
      c.n = 4; c.Mo = Mo; c.No = No; c.K = M; c.A = As; c.B = Bs; c.dW = dWs; c.overwrite = m->wg_overwrite ? 1 : 0; c.stream = sd;
      const int rc = gemm_f32_wgrad_group(c, LaunchOpts{ps.stamp, 0, m->launch_reserve});
      if (rc == 0) grouped = true;
      else if (rc != UNITER_E_SHAPE) return rc;
    }
    if (!grouped) {
    UCHECK_RC(gemm(m, UNITER_K_GEMM_WGRAD, sd, 1, 1, H, I, M, g2.f, H, lb.hact, I, m->LG(l, L_W2), I, UNITER_EPI_NONE,
                   nullptr, nullptr, nullptr, 0, wb));
    UCHECK_RC(gemm(m, UNITER_K_GEMM_WGRAD, sd, 1, 1, I, H, M, lb.du, I, lb.y1, H, m->LG(l, L_W1), H, UNITER_EPI_NONE,
                   nullptr, nullptr, nullptr, 0, wb));
    if (!fuse_db1) UCHECK_RC(uniter_colsum_f32(lb.du, M, I, I, m->LG(l, L_B1), 1, pl.col_ws, pl.col_ws_bytes, sd));
    UCHECK_RC(gemm(m, UNITER_K_GEMM_WGRAD, sd, 1, 1, H, H, M, g1.f, H, lb.ctx, H, m->LG(l, L_OW), H, UNITER_EPI_NONE,
                   nullptr, nullptr, nullptr, 0, wb));
    UCHECK_RC(gemm(m, UNITER_K_GEMM_WGRAD, sd, 1, 1, 3 * H, H, M, lb.dqkv, 3 * H, x.f, H, m->LG(l, L_QW), H,
                   UNITER_EPI_NONE, nullptr, nullptr, nullptr, 0, wb));
    }
  }
  if (!fused_qb) UCHECK_RC(uniter_colsum_f32(lb.dqkv, M, 3 * H, 3 * H, m->LG(l, L_QB), 1, pl.col_ws, pl.col_ws_bytes, sd));
  if (sd != st) UCHECK_HIP(hipEventRecord(m->ev_side[l], sd));
  return 0;
}

extern "C" int uniter_model_backward_embed(uniter_model_t* m) {
  UCHECK_ARG(m, "backward_embed: null model");
  m->launch_reserve = m->cu_reserve;
  if (!m->bwd_open) { uniter_set_error("backward_embed: call uniter_model_backward_begin first"); return UNITER_E_STATE; }
  const uniter_config_t& c = m->cfg;
  const int H = c.hidden_size;
  Plan& pl = m->plan;
  const uniter_batch_t& b = m->batch;
  const int B = pl.B, T = pl.T, R = pl.R, L = pl.L, S = pl.S;
  const float ph = pl.mode == 1 ? c.hidden_dropout_prob : 0.f;
  hipStream_t st = m->st, sd = m->side;
  const float* demb = pl.layers[0].dx;
  const bool joint = pl.has_txt && pl.has_img;
  if (pl.packed) {
    UCHECK_HIP(hipMemsetAsync(pl.dcat, 0, (size_t)B * S * H * sizeof(float), st));
    UCHECK_RC(uniter_row_scatter_add(demb, b.pack_src, pl.dcat, pl.M, H, B * S, st));
  } else {
    UCHECK_RC(uniter_gather_rows_bwd(demb, joint ? b.gather_index : nullptr, pl.dcat, B, S, L, H, st));
  }
  // Round 6: with an auxiliary stream the text branch (and, behind the image rows' pass, the region projection's bias column sums)
  // runs there, beside the image branch; batches with mixed token-type ids (one side explicit, the other implicit) keep one stream,
  // whose order serializes the two writers of the token-type table's gradient.  UNITER_EMBED_BWD_PAR=0 keeps one stream (switches.h)
  const bool par_env = uniter_switches().embed_bwd_par;
  // The order-fixed passes (uniter_model_set_deterministic) add to the token-type table by plain read-modify-writes: side by side
  // only where the two branches touch different rows (both id arrays NULL: text row 0, regions row 1); else one stream, text then image
  const bool types_alike = pl.det ? (b.txt_type_ids == nullptr && b.img_type_ids == nullptr)
                                  : (b.txt_type_ids == nullptr) == (b.img_type_ids == nullptr);
  hipStream_t ax = (par_env && m->aux && m->aux != st && m->aux != sd && pl.has_txt && pl.has_img && types_alike) ? m->aux : nullptr;
  if (ax) {
    if (!m->ev_emb0) UCHECK_HIP(hipEventCreateWithFlags(&m->ev_emb0, hipEventDisableTiming));
    if (!m->ev_emb1) UCHECK_HIP(hipEventCreateWithFlags(&m->ev_emb1, hipEventDisableTiming));
    if (!m->ev_emb2) UCHECK_HIP(hipEventCreateWithFlags(&m->ev_emb2, hipEventDisableTiming));
    UCHECK_HIP(hipEventRecord(m->ev_emb0, st));               // dcat is complete
    UCHECK_HIP(hipStreamWaitEvent(ax, m->ev_emb0, 0));
  }
  if (pl.has_txt) {
    TxtEmbedCall e = txt_embed_call(m, b, ph);      // (with the forward pass's perturbation of the word rows, where one was set)
    e.dcat = pl.dcat; e.dword = m->G(P_WORD); e.dpos = m->G(P_POS); e.dtype = m->G(P_TYPE); e.dgamma = m->G(P_ELN_G); e.dbeta = m->G(P_ELN_B);
    e.d_rows = m->ig.d_txt_rows; e.det = pl.det; e.ws = ax ? pl.emb_ws2 : pl.emb_ws; e.ws_bytes = pl.emb_ws_bytes; e.stream = ax ? ax : st;
    UCHECK_RC(txt_embed_bwd_run(e));
    if (e.d_rows) UCHECK_RC(txt_embed_bwd_rows_run(e));      // the per-token gradient: its own launch behind the text branch, on its stream
  }
  if (pl.has_img) {
    ImgEmbedCall e = img_embed_call(m, b, ph);
    e.dcat = pl.dcat; e.stats = pl.img_stats; e.d_imgfc = pl.d_imgfc; e.d_posfc = pl.d_posfc; e.dWp = m->G(P_POSL_W); e.dbp = m->G(P_POSL_B);
    e.dtype = m->G(P_TYPE); e.dg_i = m->G(P_ILN_G); e.db_i = m->G(P_ILN_B); e.dg_p = m->G(P_PLN_G); e.db_p = m->G(P_PLN_B);
    e.dg_f = m->G(P_FLN_G); e.db_f = m->G(P_FLN_B); e.det = pl.det; e.ws = pl.emb_ws; e.ws_bytes = pl.emb_ws_bytes; e.stream = st;
    UCHECK_RC(img_embed_bwd_run(e));
    const float* feat = b.img_masks ? pl.feat_eff : b.img_feat;
    // NOT pl.col_ws: the side stream's bias-gradient reductions of layer 0 may still be using it
    if (ax) {      // the region projection's bias column sums beside its weight gradient: behind the text branch on the auxiliary stream
      UCHECK_HIP(hipEventRecord(m->ev_emb1, st));             // d_imgfc is written
      UCHECK_HIP(hipStreamWaitEvent(ax, m->ev_emb1, 0));
      UCHECK_RC(uniter_colsum_f32(pl.d_imgfc, B * R, H, H, m->G(P_IMG_B), 1, pl.emb_ws3, pl.emb_ws_bytes, ax));
    }
    UCHECK_RC(gemm(m, UNITER_K_GEMM_WGRAD, st, 1, 1, H, c.img_dim, B * R, pl.d_imgfc, H, feat, c.img_dim,
                   m->G(P_IMG_W), c.img_dim, UNITER_EPI_NONE, nullptr, nullptr, nullptr, 0, 1));
    if (!ax) UCHECK_RC(uniter_colsum_f32(pl.d_imgfc, B * R, H, H, m->G(P_IMG_B), 1, pl.emb_ws, pl.emb_ws_bytes, st));
    if (b.img_masks || m->ig.d_img_feat) {
      // d(img_feat + mask_emb[img_masks]) = d_imgfc @ W_img; row 1 of mask_embedding sums the masked rows.  The same product is the
      // gradient of img_feat: formed once, in the caller's buffer when it asked for it (uniter_model_set_input_grads)
      float* d_feat = m->ig.d_img_feat ? m->ig.d_img_feat : pl.d_feat;
      UCHECK_RC(gemm(m, UNITER_K_GEMM_DGRAD, st, 0, 1, B * R, c.img_dim, H, pl.d_imgfc, H, m->P(P_IMG_W),
                     c.img_dim, d_feat, c.img_dim, UNITER_EPI_NONE, nullptr, nullptr, nullptr, 0, 0));
      if (b.img_masks) UCHECK_RC(launch_masked_rowsum(d_feat, b.img_masks, m->G(P_MASK_EMB) + c.img_dim, B * R, c.img_dim, st));
    }
    if (m->ig.d_img_pos_feat) UCHECK_RC(uniter_pos_feat_dgrad(pl.d_posfc, m->P(P_POSL_W), m->ig.d_img_pos_feat, B * R, H, st));
  }
  if (ax) {           // join the auxiliary stream's branch
    UCHECK_HIP(hipEventRecord(m->ev_emb2, ax));
    UCHECK_HIP(hipStreamWaitEvent(st, m->ev_emb2, 0));
  }
  return uniter_model_backward_end(m);
}

// Closes a backward pass: uniter_model_backward_embed ends here, and a pass that stops above a frozen prefix (include/uniter_hip.h)
// calls it in place of the embeddings' backward.
extern "C" int uniter_model_backward_end(uniter_model_t* m) {
  UCHECK_ARG(m, "backward_end: null model");
  if (!m->bwd_open) { uniter_set_error("backward_end: call uniter_model_backward_begin first"); return UNITER_E_STATE; }
  hipStream_t st = m->st, sd = m->side;
  const int nl = m->cfg.num_hidden_layers;
  if (sd != st) {   // join: everything the caller does next on `stream` sees all gradients
    UCHECK_HIP(hipEventRecord(m->ev_side[nl], sd));
    UCHECK_HIP(hipStreamWaitEvent(st, m->ev_side[nl], 0));
  }
  m->bwd_open = false;
  m->wg_overwrite = false;       // one backward pass: the next one accumulates again
  m->ig = uniter_model::InputGrads();      // ... and the input gradients were this pass's (uniter_model_set_input_grads)
  m->ag = uniter_model::AttnGrads();       // ... and so was the attention-gradient capture (uniter_model_set_attn_grads)
  // (Plan::head_rows stays: it says which of the plan's buffers the forward pass wrote, until the next forward pass remakes the plan)
  return 0;
}

extern "C" int uniter_model_set_cu_reserve(uniter_model_t* m, int cus) {
  UCHECK_ARG(m && cus >= 0 && cus <= 128, "set_cu_reserve: 0 .. 128 CUs");
  m->cu_reserve = cus;
  return 0;
}

extern "C" int uniter_model_set_deterministic(uniter_model_t* m, int on) {
  UCHECK_ARG(m, "set_deterministic: null model");
  m->deterministic = on != 0;
  return 0;
}

// What of the last forward's plan runs no arrival-ordered sum (UNITER_DET_*; 0 with the switch off or behind an inference pass).
// The embedding passes, the attention kernels' bias partials and the column sums are order-fixed in every schedule a deterministic
// plan can take; the dense products are one adder per element everywhere except on the balanced walk of the fp32x3 products
// (UNITER_X3_BALANCED, a lab switch: its partial tiles meet through a workspace in an order that was not audited), which clears the
// GEMM bit -- and the COLSUM bit with it when the riders' reductions ride on such a launch.
extern "C" int uniter_model_deterministic_coverage(const uniter_model_t* m) {
  if (!m || !m->deterministic || !m->plan.det || m->plan.mode == 0) return 0;
  const Plan& pl = m->plan;
  int mask = UNITER_DET_EMBED | UNITER_DET_ATTN | UNITER_DET_COLSUM | UNITER_DET_GEMM;
  if (pl.sk_main || pl.sk_side) mask &= ~UNITER_DET_GEMM;
  if (pl.sk_side) mask &= ~UNITER_DET_COLSUM;
  return mask;
}

extern "C" int uniter_model_set_aux_stream(uniter_model_t* m, void* aux_stream) {
  UCHECK_ARG(m, "set_aux_stream: null model");
  m->aux = (hipStream_t)aux_stream;
  return 0;
}

extern "C" int uniter_model_set_norm_partials(uniter_model_t* m, double* parts, size_t stride_doubles) {
  UCHECK_ARG(m && (parts == nullptr || stride_doubles > 0), "set_norm_partials: bad argument");
  m->norm_parts = parts;
  m->norm_stride = parts ? stride_doubles : 0;
  return 0;
}

extern "C" int uniter_model_set_input_grads(uniter_model_t* m, const float* txt_delta, float* d_txt_rows, float* d_img_feat,
                                            float* d_img_pos_feat) {
  UCHECK_ARG(m, "set_input_grads: null model");
  m->ig_next.txt_delta = txt_delta; m->ig_next.d_txt_rows = d_txt_rows; m->ig_next.d_img_feat = d_img_feat;
  m->ig_next.d_img_pos_feat = d_img_pos_feat;
  return 0;
}

extern "C" int uniter_model_set_attn_probs(uniter_model_t* m, float* out, size_t layer_stride_elems, int head_mean) {
  UCHECK_ARG(m, "set_attn_probs: null model");
  UCHECK_ARG(((uintptr_t)out & 3) == 0, "set_attn_probs: out must be 4-byte aligned");
  m->ap_next.out = out; m->ap_next.stride = out ? layer_stride_elems : 0; m->ap_next.head_mean = head_mean ? 1 : 0;
  return 0;
}

extern "C" int uniter_model_set_head_rows(uniter_model_t* m, int on) {
  UCHECK_ARG(m, "set_head_rows: null model");
  m->head_rows_next = on != 0;
  return 0;
}

extern "C" int uniter_model_set_attn_grads(uniter_model_t* m, float* out, size_t layer_stride_elems, int reduce, float* head_sums, void* ws,
                                           size_t ws_bytes) {
  UCHECK_ARG(m, "set_attn_grads: null model");
  UCHECK_ARG((((uintptr_t)out | (uintptr_t)head_sums | (uintptr_t)ws) & 3) == 0, "set_attn_grads: out, head_sums and ws must be 4-byte aligned");
  UCHECK_ARG(out || !head_sums, "set_attn_grads: head_sums without out");
  UCHECK_ARG(!head_sums || ws, "set_attn_grads: head_sums needs a workspace (uniter_attn_grad_ws_bytes)");
  m->ag_next = uniter_model::AttnGrads();
  if (out) {
    m->ag_next.out = out; m->ag_next.stride = layer_stride_elems; m->ag_next.reduce = reduce ? 1 : 0;
    m->ag_next.head_sums = head_sums; m->ag_next.ws = ws; m->ag_next.ws_bytes = ws_bytes;
  }
  return 0;
}

extern "C" int uniter_model_norm_partials_per_layer(const uniter_model_t* m) {
  if (!m) return 0;
  if (!m->plan.copies()) return 0;
  // (answers for the plan of the LAST forward: its grouped launch -- very long batches of precision 2 keep stream-K --, its row count
  // as the reduction length, its workspace of the balanced walk.  An upper bound over layers: layer 1's grid, one workgroup per CU,
  // where layer 0's balanced grid fills fewer slots)
  // Reserve 0, whatever pass ran last on this handle: the count the trainer sizes its slot buffer with, asked after the forward pass (or
  // before backward_begin), when no CU is reserved.  A backward pass that leaves CUs free runs a smaller grid and fills fewer slots.
  const WgradGroup g = wgrad_group(m, m->plan, 1, 0);
  if (!g.riders || (m->plan.prec == PREC_BF16 && m->plan.mode == 0)) return 0;
  //  a plan whose joint length is beyond the fused query|key|value bias partials (L > uniter_attn_varlen_max_len(), or
  // UNITER_ATTN_SPLIT=0) writes that bias gradient by a separate column-sum launch BEHIND the riders' launch: its squares would reach
  // no slot.  Such a plan announces no slots at all -- the caller reduces the layer's bucket itself, as in the other precisions
  if (m->plan.mode != 0 && m->plan.attn_bwd == ATTN_F32) return 0;
  return g.slots;
}

extern "C" int uniter_model_set_wgrad_overwrite(uniter_model_t* m, int on) {
  UCHECK_ARG(m, "set_wgrad_overwrite: null model");
  m->wg_overwrite = on != 0;
  return 0;
}

extern "C" int uniter_model_backward(uniter_model_t* m, const uniter_batch_t* b, const float* d_hidden,
                                     int all_layers, uint64_t seed, uint32_t offset, void* ws, size_t ws_bytes,
                                     void* stream, void* side_stream) {
  UCHECK_RC(uniter_model_backward_begin(m, b, d_hidden, all_layers, seed, offset, ws, ws_bytes, stream, side_stream));
  for (int l = m->cfg.num_hidden_layers - 1; l >= 0; --l) UCHECK_RC(uniter_model_backward_layer(m, l));
  return uniter_model_backward_embed(m);
}

extern "C" uint64_t uniter_model_generation(const uniter_model_t* m) { return m ? m->generation : 0; }

extern "C" int uniter_model_set_ready_events(uniter_model_t* m, void* const* events, int n) {
  UCHECK_ARG(m && (n == 0 || (events && (n == m->cfg.num_hidden_layers + 1 || n == m->cfg.num_hidden_layers + 2))),
             "set_ready_events: need num_hidden_layers + 1 events (embeddings, layer 0 ..), one more (the word table, last) or n = 0");
  m->ready.clear();
  for (int i = 0; i < n; ++i) {
    UCHECK_ARG(events[i], "set_ready_events: event %d is NULL", i);
    m->ready.push_back((hipEvent_t)events[i]);
  }
  return 0;
}

extern "C" int uniter_model_set_weight_mirror(uniter_model_t* m, const float* flat_base, const void* mirror_bf16,
                                              size_t numel) {
  UCHECK_ARG(m, "set_weight_mirror: null model");
  if (!mirror_bf16) { m->mirror = nullptr; m->mirror_base = nullptr; m->mirror_numel = 0; return 0; }
  UCHECK_ARG(flat_base && numel > 0, "set_weight_mirror: bad argument");
  const uniter_config_t& c = m->cfg;
  static const int ws[4] = {L_QW, L_OW, L_W1, L_W2};
  for (int l = 0; l < c.num_hidden_layers; ++l)
    for (int k = 0; k < 4; ++k) {
      const float* p = m->LP(l, ws[k]);
      UCHECK_ARG(p >= flat_base && p < flat_base + numel && (((uintptr_t)(p - flat_base) * 2) & 15) == 0,
                 "set_weight_mirror: layer %d weight %d is not inside the flat buffer on a 16-byte bf16 boundary", l, k);
    }
  m->mirror = (const unsigned short*)mirror_bf16; m->mirror_base = flat_base; m->mirror_numel = numel;
  return 0;
}

extern "C" int uniter_model_set_weight_pairing(uniter_model_t* m, int on) {
  UCHECK_ARG(m, "set_weight_pairing: null model");
  UCHECK_SHAPE(!on || (m->cfg.hidden_size % 64 == 0 && m->cfg.intermediate_size % 64 == 0),
               "set_weight_pairing: hidden and intermediate sizes must be multiples of 64 (a 64-element chunk of the optimizer is two whole 32-element units of one row)");
  m->mirror_paired = on != 0;
  return 0;
}

extern "C" int uniter_model_set_precision(uniter_model_t* m, int precision) {
  UCHECK_ARG(m && precision >= 0 && precision <= 3, "set_precision: 0 (fp32), 1 (bf16 MFMA, fp32 operands), 2 (bf16-resident operands) "
             "or 3 (fp32 from three bf16 pieces)");
  UCHECK_ARG(precision < 2 || m->mirror, "set_precision: precision 2 / 3 needs uniter_model_set_weight_mirror first");
  UCHECK_SHAPE(precision != 3 || (m->cfg.intermediate_size % 32 == 0 && m->cfg.hidden_size % 32 == 0),
               "set_precision: the fp32x3 mode needs hidden_size and intermediate_size %% 32 == 0 (got %d, %d): every forward and "
               "input-gradient product runs on 32-deep k-tiles", m->cfg.hidden_size, m->cfg.intermediate_size);
  UCHECK_SHAPE(precision != 3 || 2 * m->mirror_numel * 2 + (size_t)4096 * m->cfg.intermediate_size * 2 < (1ull << 31),
               "set_precision: the fp32x3 mode addresses the weight pieces with 31-bit offsets (%zu parameters are too many)", m->mirror_numel);
  UCHECK_SHAPE(precision != 2 || (m->cfg.intermediate_size % 64 == 0 && m->cfg.hidden_size % 64 == 0),
               "set_precision: the bf16-resident mode needs hidden_size and intermediate_size %% 64 == 0 (got %d, %d): every "
               "forward and input-gradient product runs on 64-deep k-tiles", m->cfg.hidden_size, m->cfg.intermediate_size);
  m->precision = (Precision)precision;
  return 0;
}

extern "C" int uniter_prof_enable(uniter_model_t* m, int kind) {
  UCHECK_ARG(m && kind >= -1 && kind < UNITER_K_COUNT, "prof_enable: bad argument");
  m->prof_kind = kind;
  m->prof_used = 0;
  const size_t want = kind < 0 ? 65536 : 8192;       // event pairs x 2: ~220 timed launches per step when every kind is on
  if (kind && m->prof_ev.size() < want) {
    const size_t have = m->prof_ev.size();
    m->prof_ev.resize(want);
    m->prof_tag.resize(want / 2);
    for (size_t i = have; i < want; ++i) UCHECK_HIP(hipEventCreate(&m->prof_ev[i]));
  }
  return 0;
}

extern "C" int uniter_prof_enable_stamps(uniter_model_t* m, int on, void* stream) {
  UCHECK_ARG(m, "prof_enable_stamps: null model");
  const size_t cap = 1 << 14;                        // launches; 16 KB each
  const size_t bytes = cap * 2 * STAMP_WGS * sizeof(unsigned long long);
  if (on && !m->stamp_buf) {
    UCHECK_HIP(hipMalloc((void**)&m->stamp_buf, bytes));
    m->stamp_cap = cap;
    m->stamp_tag.resize(cap);
  }
  if (on) {
    UCHECK_HIP(hipMemset(m->stamp_buf, 0, bytes));   // 0 = workgroup did not run (the clock never reads 0)
    m->stamp_used = 0;
  } else if (m->stamp_buf) {
    (void)hipFree(m->stamp_buf);
    m->stamp_buf = nullptr; m->stamp_cap = m->stamp_used = 0;
  }
  (void)stream;
  return 0;
}

extern "C" int uniter_prof_collect_stamps(uniter_model_t* m, int* n_launches, double* total_ms, int n_kinds) {
  UCHECK_ARG(m && n_launches && total_ms && n_kinds >= UNITER_K_COUNT, "prof_collect_stamps: need UNITER_K_COUNT slots");
  for (int k = 0; k < n_kinds; ++k) { n_launches[k] = 0; total_ms[k] = 0.0; }
  if (!m->stamp_buf || m->stamp_used == 0) return 0;
  UCHECK_HIP(hipDeviceSynchronize());
  const size_t per = (size_t)2 * STAMP_WGS;
  std::vector<unsigned long long> h(m->stamp_used * per);
  UCHECK_HIP(hipMemcpy(h.data(), m->stamp_buf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < m->stamp_used; ++i) {
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int w = 0; w < STAMP_WGS; ++w) {
      const unsigned long long a = h[i * per + w], b = h[i * per + STAMP_WGS + w];
      if (a && a < t0) t0 = a;
      if (b > t1) t1 = b;
    }
    if (t0 == ~0ull || t1 < t0) continue;                  // the scope launched no stamped kernel
    n_launches[m->stamp_tag[i]] += 1;
    total_ms[m->stamp_tag[i]] += (double)(t1 - t0) * 1e-5;  // 100 MHz ticks -> ms
  }
  return 0;
}

// every stamped launch in launch order: kind and [first workgroup's start, last workgroup's end] in microseconds since the
// first stamped launch's start (the GPU's 100-MHz clock): where on the step's time axis each GEMM sits, with nothing added to
// the streams -- e.g. how long the chip takes from the last backward GEMM of a step to the first forward GEMM of the next
extern "C" int uniter_prof_stamp_spans(uniter_model_t* m, int* kinds, double* start_us, double* end_us, int cap, int* n) {
  UCHECK_ARG(m && kinds && start_us && end_us && n && cap >= 0, "prof_stamp_spans: null pointer");
  *n = 0;
  if (!m->stamp_buf || m->stamp_used == 0) return 0;
  UCHECK_HIP(hipDeviceSynchronize());
  const size_t per = (size_t)2 * STAMP_WGS;
  std::vector<unsigned long long> h(m->stamp_used * per);
  UCHECK_HIP(hipMemcpy(h.data(), m->stamp_buf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  unsigned long long base = 0;
  for (size_t i = 0; i < m->stamp_used && *n < cap; ++i) {
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int w = 0; w < STAMP_WGS; ++w) {
      const unsigned long long a = h[i * per + w], b = h[i * per + STAMP_WGS + w];
      if (a && a < t0) t0 = a;
      if (b > t1) t1 = b;
    }
    if (t0 == ~0ull || t1 < t0) continue;
    if (*n == 0) base = t0;
    kinds[*n] = m->stamp_tag[i];
    start_us[*n] = ((double)t0 - (double)base) * 1e-2;
    end_us[*n] = ((double)t1 - (double)base) * 1e-2;
    ++*n;
  }
  return 0;
}

// milliseconds during which at least one stamped launch of a kind in `kind_mask` (bit k = UNITER_K_* k) was running:
// the union of the launches' [first start, last end] intervals -- what two streams that share the chip took TOGETHER
extern "C" int uniter_prof_stamps_union(uniter_model_t* m, unsigned kind_mask, double* union_ms) {
  UCHECK_ARG(m && union_ms, "prof_stamps_union: null pointer");
  *union_ms = 0.0;
  if (!m->stamp_buf || m->stamp_used == 0) return 0;
  UCHECK_HIP(hipDeviceSynchronize());
  const size_t per = (size_t)2 * STAMP_WGS;
  std::vector<unsigned long long> h(m->stamp_used * per);
  UCHECK_HIP(hipMemcpy(h.data(), m->stamp_buf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<std::pair<unsigned long long, unsigned long long>> iv;
  for (size_t i = 0; i < m->stamp_used; ++i) {
    if (!((kind_mask >> m->stamp_tag[i]) & 1u)) continue;
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int w = 0; w < STAMP_WGS; ++w) {
      const unsigned long long a = h[i * per + w], b = h[i * per + STAMP_WGS + w];
      if (a && a < t0) t0 = a;
      if (b > t1) t1 = b;
    }
    if (t0 != ~0ull && t1 >= t0) iv.emplace_back(t0, t1);
  }
  std::sort(iv.begin(), iv.end());
  unsigned long long tot = 0, cs = 0, ce = 0;
  bool open = false;
  for (auto& p : iv) {
    if (!open) { cs = p.first; ce = p.second; open = true; }
    else if (p.first > ce) { tot += ce - cs; cs = p.first; ce = p.second; }
    else if (p.second > ce) ce = p.second;
  }
  if (open) tot += ce - cs;
  *union_ms = (double)tot * 1e-5;
  return 0;
}

extern "C" int uniter_prof_collect_kinds(uniter_model_t* m, int* n_launches, double* total_ms, int n_kinds) {
  UCHECK_ARG(m && n_launches && total_ms && n_kinds >= UNITER_K_COUNT, "prof_collect_kinds: need UNITER_K_COUNT slots");
  for (int k = 0; k < n_kinds; ++k) { n_launches[k] = 0; total_ms[k] = 0.0; }
  for (size_t i = 0; i + 1 < m->prof_used; i += 2) {
    UCHECK_HIP(hipEventSynchronize(m->prof_ev[i + 1]));
    float ms = 0.f;
    UCHECK_HIP(hipEventElapsedTime(&ms, m->prof_ev[i], m->prof_ev[i + 1]));
    const int k = m->prof_tag[i / 2];
    n_launches[k] += 1;
    total_ms[k] += ms;
  }
  m->prof_used = 0;
  return 0;
}

extern "C" int uniter_prof_collect(uniter_model_t* m, int* n_launches, double* total_ms) {
  UCHECK_ARG(m && n_launches && total_ms, "prof_collect: null pointer");
  double tot = 0.0;
  int n = 0;
  for (size_t i = 0; i + 1 < m->prof_used; i += 2) {
    UCHECK_HIP(hipEventSynchronize(m->prof_ev[i + 1]));
    float ms = 0.f;
    UCHECK_HIP(hipEventElapsedTime(&ms, m->prof_ev[i], m->prof_ev[i + 1]));
    tot += ms;
    ++n;
  }
  *n_launches = n; *total_ms = tot;
  m->prof_used = 0;
  return 0;
}
