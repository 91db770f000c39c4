// Every environment switch of the C library, in one table: name, parse, default, and the measurement behind the default.
// uniter_switches() fills the table from the environment at its FIRST USE (not at library load) and never again: a process
// sees one schedule for its whole life, and a test of another schedule starts a child process with the variable set
// (tests/test_model_gpu.py::test_alternative_schedules_keep_the_golden_gradients).  switches.cpp is the only translation unit
// of the library that reads the environment; INTEGRATION.md ("Environment switches") lists the same names for users, and
// tests/test_switches_cpu.py holds the three lists together.
//
// One member per variable; the comment above a member starts with the variable's name.  Parses:
//   off-if-0  on unless the value starts with '0'            on-if-1  off unless the value starts with '1'
//   int       atoi of the value, the stated default if unset
// The Python side's switches (model.py, trainer.py, dp.py, data.py) are read at call time and are not part of this table.
#pragma once

struct Switches {
  // ---------------------------------------------------------------------------------------------- attention
  // UNITER_ATTN_PRIO (int, default 2): wave priority (s_setprio level) the attention kernels of all three files -- attention_f32.hip,
  // attention_bf16.hip, attention_x3.hip -- raise themselves to: they run on the critical path beside the side stream's weight gradients
  int attn_prio;
  // UNITER_ATTN_SPLIT (off-if-0): =0 keeps the one-wave-per-block resident kernels of attention_f32.hip (A/B measurements);
  // uniter_attn_varlen_max_len() is then 0, so no plan takes the L <= 192 kernels or the fused query|key|value bias partials
  bool attn_split;
  // UNITER_ATTN_BWD_FUSED (off-if-0): =0 runs the two passes of the L <= 192 backward as two launches (A/B measurements), in
  // attention_f32.hip and attention_bf16.hip alike
  bool attn_bwd_fused;
  // UNITER_ATTN_X3 (off-if-0): precision 3: the attention's products on the bf16 pipe too (csrc/attention_x3.hip) -- L <= 192 and, with
  // dropout, keep flags drawn ahead of the kernel.  =0 keeps the fp32-MFMA kernels of attention_f32.hip (A/B measurements).
  bool attn_x3;
  // UNITER_ATTN_B16X (off-if-0): precision 2: the bf16 attention in attention_x3.hip's decomposition (no scratch hand-over).  =0 keeps
  // attention_bf16.hip's kernels (A/B measurements).
  bool attn_b16x;
  // UNITER_DCTX_SPLIT (off-if-0): precision 3 with the x3 attention backward: the attention-output input gradient leaves as k-pieces
  // (the kernel sums them).  A/B switch
  bool dctx_split;
  // UNITER_KEEP_PREGEN (off-if-0): dropout keep flags of the attention probabilities of ALL layers, drawn in one elementwise launch
  // ahead of everything -- a function of (seed, offset) alone, so it runs while the optimizer still streams the word table the text
  // branch waits for (the L <= 192 kernels then read them; the backward pass reads the same words).  =0: the kernels draw them
  bool keep_pregen;
  // UNITER_HIDDEN_PREGEN (on-if-1): the hidden dropout's keep flags (the two dropout + residual + LayerNorm passes of every layer,
  // forward AND backward) behind the attention's on the same stream: built, bit-identical (tests/test_layernorm_gpu.py) and OFF by
  // default.  Alone a row pass is 1.5 / 1.8 us faster without its ten Philox rounds per group; in the step it is not -- there the
  // passes wait for memory, the Philox rounds run in that shadow, and the generator launch is one more kernel beside the forward's
  // head: 9.87 / 9.87 ms without against 9.96 / 9.86 with (fp32x3), 4.58 / 4.60 against 4.60 / 4.61 (bf16), two same-box pairs each
  bool hidden_pregen;

  // ------------------------------------------------------------------------------- forward pass, embeddings
  // UNITER_GELU_D (off-if-0): the FFN-up epilogue stores gelu'(u) instead of u.  =0: A/B switch (store the pre-activation, libm erf
  // twice); precision 3 always stores gelu'(u)
  bool gelu_d;
  // UNITER_IMG_SK (off-if-0): region-feature projection (model/model.py:267): 576 x 768 outputs are 108 tiles of 64 x 64 for 1024
  // workgroup slots with K = 2048 -- as a stream-K accumulation on top of the bias rows it fills the chip (fp32: 58 -> 25 us).
  // Native fp32 only: the float atomics make the sum's order vary from run to run -- 1e-7 in fp32, but the bf16 mode amplifies any
  // such difference through its rounding stages, DESIGN.md section 2, and the fp32x3 mode's forward and backward are bit-reproducible
  // run to run, which tests/test_model_gpu.py::test_cu_reserve_for_a_gradient_exchange_changes_no_result relies on -- round 6 tried
  // the stream-K form there and took it out again for that reason
  bool img_sk;
  // UNITER_GATHER_EX (off-if-0): (round 6) the joint rows and their operand copy for layer 0's first product in ONE launch
  // (precisions 2 / 3, unpacked): this chain -- text embeddings, gather, split -- is what the first encoder product waits for behind
  // the optimizer's update of the word table
  bool gather_ex;
  // UNITER_EMBED_BWD_PAR (off-if-0): Round 6: the tail of the step is a chain of latency-bound launches behind the last input gradient
  // (text-embedding backward 55 us, image-embedding backward 67, the 7-d projection's and the region projection's weight gradients
  // 15 + 52, column sums: 220 us on one stream, profiles/r06_timeline_f32x3.txt), while layer 0's weight-gradient launch holds most of
  // the chip on the side stream.  The text branch and the image branch share nothing but dcat: with an auxiliary stream the text
  // branch (and, behind the image rows' pass, the region projection's bias column sums) runs there, beside the image branch.  Same
  // kernels, same results; the token-type table's gradient is the one buffer both branches add to (row 0 / the text rows' types there,
  // row 1 / the image rows' types here): with explicit type ids on both sides both scatter by float atomics, without them on either
  // side each finalizes into its own row, and in those two cases no ordering between the branches is needed.  With mixed ids (one side
  // explicit, the other implicit) one branch's atomics land on the row the other finalizes with a plain read-add-write, which could
  // lose an update: those batches keep one stream, whose order serializes the two writers.  =0 keeps one stream.
  bool embed_bwd_par;

  // ------------------------------------------------------------------- wave priority of the main stream's GEMMs
  // UNITER_MAIN_PRIO (int, default 0): wave priority of the critical path's GEMMs over the side stream's weight gradients (common.h: LaunchOpts::prio).
  // fp32: measured WORSE (14.09 against 13.73 ms per step with level 2: the input-gradient GEMM then starves the weight-gradient
  // launch it shares the matrix pipe with, and the chain waits for that launch at the layer's end), so the default is 0 here
  int main_prio;
  // UNITER_MAIN_PRIO_BF16 (int, default 2): the same for the bf16-resident GEMMs, which gain 0.6 % from level 2 (their bound is operand
  // staging, not the pipe)
  int main_prio_bf16;
  // UNITER_MAIN_PRIO_X3 (int, default 0): the same for the x3 products of precision 3
  int main_prio_x3;

  // -------------------------------------------------------------------------- native fp32 GEMMs (gemm_f32.hip)
  // UNITER_GEMM_SK (int, default 1): stream-K when the tiles fill the slots unevenly (only legal for a plain accumulating GEMM):
  // 0 never, 1 heuristic, 2 whenever legal
  int gemm_sk;
  // UNITER_WGRAD_SLOTS_F32 (int, default 0 = the heuristic's): A/B: pieces of the stream-K form
  int wgrad_slots_f32;
  // UNITER_WGRAD_CFG (int, default 0): weight gradients: 21 selects 128 x 128 stream-K tiles (measured slower: DESIGN.md section 9),
  // 24 the 64 x 64 ones
  int wgrad_cfg;
  // UNITER_WGRAD_WHOLE (int, default 15): bit mask over a layer's weight gradients by output shape (1: [H, I] output.dense, 2: [I, H]
  // intermediate.dense, 4: [H, H] attention output, 8: [3H, H] query|key|value): whole-K tiles (cfg 25) instead of stream-K.
  // Default 15: measured 13.95 against 14.06 ms per step with every shape on whole tiles -- the k-synchronous tiles of a
  // tile row share their operand panel in L2 (the LayerNorm backward beside them runs at 17 instead of 26 us) -- and
  // without float atomics the fp32 weight gradients are bit-reproducible and a first backward pass may overwrite them.
  int wgrad_whole;
  // UNITER_WGRAD_GROUP_F32 (int, default 2): =1: EVERY layer's four weight gradients as ONE persistent launch of whole-K tiles (1728
  // tiles for 1024 slots, uniter_wgrad_f32_group).  Measured (three same-box pairs): the launch itself runs at 0.47-0.49 of the fp32
  // peak in situ (four launches: 0.39), both gradient families together at 0.78 (0.67), the attention backward beside it at 97
  // instead of 151 us -- and the STEP is 0.7-1.1 % slower (13.87-13.90 vs 13.72-13.75 ms): its 1024 resident workgroups
  // hold every CU's LDS for 370 us, and each kernel of the input-gradient chain queues for slots before its first
  // workgroup starts (a wait no per-launch figure shows).  So layers nl-1 .. 1 keep four launches.
  // Layer 0 is the exception (= 2, the default; 0 = never, 1 = every layer): its weight gradients run
  // BEHIND the input-gradient chain, alone on the chip, where four launches of 576 / 576 / 144 / 432 tiles leave a quarter
  // of the 1024 slots idle and one balanced launch does not: 13.69 -> 13.55 ms per step (three same-box pairs).
  // (The grouped launch needs every shape on whole tiles: UNITER_WGRAD_WHOLE = 15 and UNITER_WGRAD_CFG = 0.)
  int wgrad_group_f32;
  // UNITER_WGRAD_GROUP_F32_SLOTS (int, default 1024; values below 8 mean 1024, others round down to a multiple of 8): grid cap of that
  // grouped launch
  int wgrad_group_f32_slots;

  // ----------------------------------------------------------------------------------- precision 2 (bf16-resident)
  // UNITER_B16_PERSIST (int, default 0): precision 2, round 6: which products run on the persistent loader / compute kernels of
  // gemm_bf16_p.hip where they win isolated (profiles/r06_b1p_lab.txt): the query|key|value projection on 128 x 192 tiles (252 for 256
  // CUs: 15.4 against 16.9 us), the N = hidden products with k-pieces on persistent 128 x 128 tiles (FFN-down forward 20.4 against
  // 22.6 us, FFN-up / QKV input gradients 22.1 / 19.1 against 24.1 / 20.5).  The N = intermediate products tie (128 x 256 tiles stage
  // a quarter less per k-tile -- 0.75 against 0.93 us, the vendor library's slope -- and pay 2 us more fixed cost on a 12-k-tile loop):
  // they keep gemm_dma_kernel.  A bit mask: 1 = QKV forward, 2 = N = hidden products, 4 = the grouped weight gradients (216 whole-K
  // tiles of 128 x 256 -- 47 against 61 us alone), 8 = the wide products as well.
  // Default 0: built, parity-tested through the C ABI, faster isolated -- and the STEP is slower with every subset of them (same-box
  // A/B, profiles/r06_b16_persist_ab.txt: 4.39 ms with none, 4.43-4.75 with bits 1 / 2 / 4 / 7 / 12 / 15): their 96-144 KB workgroups
  // own a CU, where two 64-KB workgroups of gemm_dma_kernel let the two backward streams and the kernel boundaries of the forward
  // pass overlap
  int b16_persist;
  // UNITER_B16_RIDERS (first character of the value; 0 = unset): precision 2: the riders of the fp32x3 mode (UNITER_X3_RIDERS) on the
  // grouped bf16 weight-gradient launch -- built, parity-tested, and OFF by default ('1' switches them on): measured 4.42 -> 4.51 ms
  // per step, two same-box pairs.  In this mode the two backward streams really overlap (two 64-KB workgroups share a CU) and the
  // weight-gradient stream idles half of every layer: the separate column-sum / finalize / sum-of-squares launches cost the step
  // nothing there, while the riders lengthen the launch the input-gradient chain shares its CUs with (the fp32x3 mode is the opposite
  // case: its streams serialise, every launch is step time).
  // Round 6: with the grouped launch on the persistent 128 x 256-tile kernel (UNITER_B16_PERSIST bit 4) a workgroup of it owns its CU,
  // the two backward streams time-slice as in the fp32x3 mode, and every side launch is step time: there the riders are ON unless the
  // value starts with '0'
  char b16_riders;
  // UNITER_WGRAD_GROUP (int, default 1): 1: the four weight gradients of a layer as one launch of whole-K tiles (gemm_bf16_dma.hip);
  // 0: four stream-K launches with float atomics; 2: as 1 with the three early products launched next to the attention
  // backward (measured slower); 4: as 1 with three LDS stages (measured slower)
  int wgrad_group;
  // UNITER_WGRAD_GROUP_WGS (int rounded down to a multiple of 8, default 256): cap of that launch's grid (0 = one workgroup per
  // tile).  Default 256 = one workgroup of this launch per CU, walking its tiles: the launch alone takes what two co-resident
  // workgroups take (a lone 4-wave tile runs its k-loop at 0.57 us per k-tile against 0.93 for two), and every CU keeps a slot for the
  // other stream's kernels.  Measured again once the attention backward took its CU in one launch (four same-box rounds): UNITER-base
  // 4.75 -> 4.71 ms, UNITER-large 9.65 -> 9.49, config 5 at B = 32 8.19 -> 8.00 ms per step; 192 / 320 / 384 workgroups 4.77-4.80,
  // 128 5.13
  int wgrad_group_wgs;
  // UNITER_WGRAD_SLOTS (int, default 0 = 512): A/B: stream-K pieces of the ungrouped weight gradients (gemm_bf16.hip).  They run on the
  // side stream BESIDE the input-gradient chain: 512 pieces (two per CU, ~96 KB of LDS) leave room for a 64-KB workgroup of the other
  // stream on every CU, 768 (three per CU) fill the LDS and the two streams take turns instead (bf16 step 2898 -> 2944 samples/s;
  // 384: 2913, 256: 2798)
  int wgrad_slots;
  // UNITER_WGRAD_SLABS (on-if-1): ungrouped weight gradients dW[M, N] += dY^T X as split-K slabs + one reduce pass instead of the
  // stream-K + float-atomics kernel of gemm_bf16.hip.  Measured at K = 2624 (profiles/r02_gemm_bf16_v2.txt): 768 x 3072 39.2 -> 30.9 us
  // with two pieces, 2304 x 768 26.0 -> 24.7 (two), 768 x 768 17.9 -> 16.8 (four); 3072 x 768 stays on stream-K (29.0 vs 31.2).
  // In the training step the gain does not survive (2870 -> 2855 samples/s: the weight gradients share the chip with the
  // input-gradient chain, whose idle slots the perfectly balanced stream-K pieces fill better), so the slab form is an
  // opt-in and the default stays stream-K.
  bool wgrad_slabs;

  // ------------------------------------------------------------------------ precision 3 (fp32 from three bf16 pieces)
  // UNITER_X3_CFG (int, default 0 = the cost model's choice): tile geometry / MFMA shape of every x3 product (gemm_split3.hip), and of the
  // grouped weight-gradient launch when it carries no riders.  The riders need the default geometries: 0 or 3 (3 = 128 x 128 tiles)
  int x3_cfg;
  // UNITER_X3_CFG_FFN_UP_FWD (int, default 0 = as UNITER_X3_CFG): lab switch: the FFN-up forward product alone on another tile geometry
  // -- 3 = 128 x 128, whose workgroups leave register room for a resident optimizer wave, which the 128 x 256 geometry's 504 of 512
  // registers per SIMD do not
  int x3_cfg_ffn_up_fwd;
  // UNITER_X3_WIDE (off-if-0): =0 takes the 128 x 256 tiles (cfg 4; and with them the 128 x 192 ones) out of the cost model of
  // x3_choose (gemm_split3.hip)
  bool x3_wide;
  // UNITER_X3_192 (off-if-0): =0 takes the 128 x 192 tiles (cfg 5: forward layout, fp32 output; 60 KB staged per k-tile against the
  // 128 x 256 tile's 72 -- 1.75 us) out of that cost model
  bool x3_192;
  // UNITER_X3_BAND_H (int, default 0 = sqrt(32 BN / BM)): tile rows per band of the walk (lab switch: how many row panels an XCD's chunk
  // of the walk spans decides how often the eight L2s fetch the same operand panels -- VERDICT r04 item 7)
  int x3_band_h;
  // UNITER_X3_BALANCED (int, default 0: off; bit 0 = the grouped weight gradients, bit 1 = the forward products with a bias epilogue):
  // the balanced walk is built and parity-tested, and LOSES in the step -- 9.40 -> 9.81 ms (bit 0), 9.40 -> 9.52 (bit 1) at
  // configs[1], +0.8 % only for UNITER-large's weight gradients (384 tiles: two rounds): the CUs a 216-tile launch leaves idle are not
  // idle in the step (the other stream's input-gradient kernels take them), the hand-over costs ~4 k-tiles per workgroup, and a
  // workgroup that waits for a partial sum holds its CU (profiles/r05_balanced_walk_ab.txt)
  int x3_balanced;
  // UNITER_X3_RIDERS (off-if-0): precision 3 (round 5): the column reductions of a layer's backward, the bias gradient of
  // intermediate.dense and the layer's share of the clip norm RIDE on the grouped weight-gradient launch
  // (uniter_wgrad_x3_group_riders) -- no finalize / column-sum / sum-of-squares launches on the side stream.  =0 keeps the separate
  // launches (A/B measurements)
  bool x3_riders;
  // UNITER_X3_WGRAD_CFG (3 or 4; anything else, and the default: 4): geometry of the grouped weight-gradient launch: 4 = 128 x 256
  // tiles (round 5), 3 = 128 x 128
  int x3_wgrad_cfg;
  // UNITER_WGRAD_X3_WGS (int, default -1 = unset): n >= 0 forces a grid for every layer's grouped launch (0 = one workgroup per CU).
  // Unset, layer 0's launch -- which runs BEHIND the input-gradient chain, beside the embedding backward's row passes on the main
  // stream -- takes the smallest grid that needs no more rounds (432 tiles: 216 workgroups walk two tiles each, as 256 would) and
  // leaves 40 CUs to those passes: their 190-register waves find no room on a CU a persistent 144-KB workgroup holds (img_embed_bwd
  // 112 us for 576 rows when it has to wait for one)
  int wgrad_x3_wgs;

  // ------------------------------------------------------------------------------------ LayerNorm backward
  // UNITER_LNB_WAVES (8 if the value is 8, else 4): waves per workgroup of the backward row pass (A/B switch)
  int lnb_waves;
  // UNITER_LNB_ROWS (int, default 2, at least 1): rows per wave of that pass (A/B switch)
  int lnb_rows;
};

const Switches& uniter_switches();

// UNITER_ATTN_X3_LAB (int, default 0): measurement builds only (-DUNITER_X3_LAB, tests/tools/attn_x3_lab.py): which measurement form
// of attn_x3_bwd_kernel runs.  The one switch that is NOT in the table: the tool changes it between its timed loops inside one
// process, so it is read at every call
int uniter_switch_attn_x3_lab();
