// The one translation unit of the library that reads the environment (switches.h: what each switch selects, and why its
// default is what it is).
#include <stdlib.h>
#include "switches.h"

namespace {

bool off_if_0(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
bool on_if_1(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

Switches read_switches() {
  Switches s;
  s.attn_prio = env_int("UNITER_ATTN_PRIO", 2);
  s.attn_split = off_if_0("UNITER_ATTN_SPLIT");
  s.attn_bwd_fused = off_if_0("UNITER_ATTN_BWD_FUSED");
  s.attn_x3 = off_if_0("UNITER_ATTN_X3");
  s.attn_b16x = off_if_0("UNITER_ATTN_B16X");
  s.dctx_split = off_if_0("UNITER_DCTX_SPLIT");
  s.keep_pregen = off_if_0("UNITER_KEEP_PREGEN");
  s.hidden_pregen = on_if_1("UNITER_HIDDEN_PREGEN");
  s.gelu_d = off_if_0("UNITER_GELU_D");
  s.img_sk = off_if_0("UNITER_IMG_SK");
  s.gather_ex = off_if_0("UNITER_GATHER_EX");
  s.embed_bwd_par = off_if_0("UNITER_EMBED_BWD_PAR");
  s.main_prio = env_int("UNITER_MAIN_PRIO", 0);
  s.main_prio_bf16 = env_int("UNITER_MAIN_PRIO_BF16", 2);
  s.main_prio_x3 = env_int("UNITER_MAIN_PRIO_X3", 0);
  s.gemm_sk = env_int("UNITER_GEMM_SK", 1);
  s.wgrad_slots_f32 = env_int("UNITER_WGRAD_SLOTS_F32", 0);
  s.wgrad_cfg = env_int("UNITER_WGRAD_CFG", 0);
  s.wgrad_whole = env_int("UNITER_WGRAD_WHOLE", 15);
  s.wgrad_group_f32 = env_int("UNITER_WGRAD_GROUP_F32", 2);
  s.wgrad_group_f32_slots = env_int("UNITER_WGRAD_GROUP_F32_SLOTS", 1024);
  s.b16_persist = env_int("UNITER_B16_PERSIST", 0);
  { const char* e = getenv("UNITER_B16_RIDERS"); s.b16_riders = e ? e[0] : 0; }
  s.wgrad_group = env_int("UNITER_WGRAD_GROUP", 1);
  s.wgrad_group_wgs = env_int("UNITER_WGRAD_GROUP_WGS", 256) / 8 * 8;
  s.wgrad_slots = env_int("UNITER_WGRAD_SLOTS", 0);
  s.wgrad_slabs = on_if_1("UNITER_WGRAD_SLABS");
  s.x3_cfg = env_int("UNITER_X3_CFG", 0);
  s.x3_cfg_ffn_up_fwd = env_int("UNITER_X3_CFG_FFN_UP_FWD", 0);
  s.x3_wide = off_if_0("UNITER_X3_WIDE");
  s.x3_192 = off_if_0("UNITER_X3_192");
  s.x3_band_h = env_int("UNITER_X3_BAND_H", 0);
  s.x3_balanced = env_int("UNITER_X3_BALANCED", 0);
  s.x3_riders = off_if_0("UNITER_X3_RIDERS");
  { const int v = env_int("UNITER_X3_WGRAD_CFG", 0); s.x3_wgrad_cfg = (v == 3 || v == 4) ? v : 4; }
  s.wgrad_x3_wgs = env_int("UNITER_WGRAD_X3_WGS", -1);
  s.lnb_waves = env_int("UNITER_LNB_WAVES", 0) == 8 ? 8 : 4;
  { const int v = env_int("UNITER_LNB_ROWS", 2); s.lnb_rows = v < 1 ? 1 : v; }
  return s;
}

}  // namespace

const Switches& uniter_switches() {
  static const Switches s = read_switches();
  return s;
}

int uniter_switch_attn_x3_lab() { return env_int("UNITER_ATTN_X3_LAB", 0); }
