// k_pg instances with per-column dequant scales (PC; nqk_epilogue.s_col), nibble-packed int4
// weights: the twins of nqk_pg_inst_i4.hip
#include "nqk_pgemm_kernel.h"

namespace nqk {
bool pg_dispatch_pc4(int key, const PgArgs& x) {
  switch (key) {
    NQK_PG_CASE_PC(PG_QKV, 12, true, true, true)  // 8-bit outputs (nqk_epilogue.w_bits): the saturating store
    NQK_PG_CASE_PC(PG_QKV, 12, true, true, false)
    NQK_PG_CASE_PC(PG_GELU, 12, true, true, false)
    NQK_PG_CASE_PC(PG_GLUT, 12, true, true, false)
    NQK_PG_CASE_PC(PG_GLUT1, 12, true, true, false)
    NQK_PG_CASE_PC(PG_RESID, 12, true, true, false)
    NQK_PG_CASE_PC(PG_RESID, 12, false, true, false)
    NQK_PG_CASE_PC(PG_RESID, 48, true, true, false)
    NQK_PG_CASE_PC(PG_RESID, 48, false, true, false)
    default:
      return false;
  }
}
}  // namespace nqk
