// Error reporting / version entry points of libuniter_hip.so.
#include <stdarg.h>
#include <stdio.h>
#include "common.h"
#include "gemm_internal.h"

static thread_local char g_err[512] = "";

void uniter_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int uniter_abi_version(void) { return UNITER_ABI_VERSION; }
extern "C" const char* uniter_last_error(void) { return g_err; }
extern "C" const char* uniter_build_info(void) {
  return "libuniter_hip gfx950 fp32-mfma (built " __DATE__ " " __TIME__ ")";
}

// The NEXT attention-backward call of this host thread writes its per-sample bias partials in a fixed order (include/uniter_hip.h).
// A hand-over of the C ABI only: the public attention-backward wrappers take it as their first statement (a refused call and the forms
// that emit no bias partials included) and pass it down as AttnCall::det; the model's schedule sets that field from Plan::det
// (attn_internal.h) instead.
// One per HOST THREAD, so that two threads driving the library can never take each other's flag.
static thread_local int g_attn_bwd_next_det = 0;
extern "C" int uniter_attn_bwd_set_next_det(int on) {
  g_attn_bwd_next_det = on != 0;
  return 0;
}
bool attn_bwd_take_next_det() {
  const int d = g_attn_bwd_next_det;
  g_attn_bwd_next_det = 0;
  return d != 0;
}
