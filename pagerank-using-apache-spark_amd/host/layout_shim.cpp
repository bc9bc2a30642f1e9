// Test shim (not product code): exposes the layout policy of csrc/pr_layout.h -- class count,
// layout and geometry, entry code, hot-set size, the LDS map of k_spmv_hot -- to
// tests/test_layout_policy_cpu.py on the CPU.
#include "pr_layout.h"

extern "C" {
int prl_classes(int opt_classes, int64_t gather_bytes) { return pr::class_setting(opt_classes, gather_bytes); }
int prl_hot_slots(int opt_hot_slots) { return pr::hot_slots_setting(opt_hot_slots); }
// out: {layout, C, Q_pad, n_rows, S_pad, fits}
void prl_layout(uint32_t flags, int opt_classes, int P, int64_t n_local_max, int64_t gather_est, int64_t *out) {
  const pr::LayoutGeom l = pr::choose_layout(flags, opt_classes, P, n_local_max, gather_est);
  const int64_t v[6] = {l.layout, l.C, l.Q_pad, l.n_rows, l.S_pad, l.fits ? 1 : 0};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
}
int prl_code_one_part(int opt_codes, int P, int whole_slice, int64_t Q_pad) {
  return pr::code_one_part(opt_codes, P, whole_slice != 0, Q_pad);
}
int prl_piece_codes_allowed(int opt_codes, int P) { return pr::piece_codes_allowed(opt_codes, P) ? 1 : 0; }
// out: {code, slots}
void prl_code_of_parts(int slots, int P, int64_t vmax, int *out) {
  const pr::CodeChoice c = pr::code_of_parts(slots, P, vmax);
  out[0] = c.code;
  out[1] = c.slots;
}
int64_t prl_hot_lds_bytes(int P, int Kp, int tbl) { return (int64_t)pr::HotGeom{0, P, Kp, 0, 0, 0, tbl}.lds_bytes(); }
// out: {kHotLdsBytes, kHotSlotsMax, kHotSlotsDefault, kHotThreads, kStageSlots, kPieceTblSlots, kMaxClasses,
// kMaxPackParts, sizeof(HotGeom)}
void prl_constants(int64_t *out) {
  const int64_t v[9] = {pr::kHotLdsBytes, pr::kHotSlotsMax,    pr::kHotSlotsDefault, pr::kHotThreads,        pr::kStageSlots,
                        pr::kPieceTblSlots, pr::kMaxClasses, pr::kMaxPackParts,    (int64_t)sizeof(pr::HotGeom)};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
}
}
