// k_pg instances with per-column dequant scales (PC; nqk_epilogue.s_col), int8 weights: the
// twins of nqk_pg_inst_i8.hip, nqk_pg_inst_resid.hip and nqk_pg_inst_tiny.hip (WM = 1)
#include "nqk_pgemm_kernel.h"

namespace nqk {
bool pg_dispatch_pc(int key, const PgArgs& x) {
  switch (key) {
    NQK_PG_CASE_PC(PG_QKV, 12, true, false, true)
    NQK_PG_CASE_PC(PG_QKV, 12, true, false, false)
    NQK_PG_CASE_PC(PG_GELU, 12, true, false, false)
    NQK_PG_CASE_PC(PG_GLUT, 12, true, false, false)
    NQK_PG_CASE_PC(PG_GLUT1, 12, true, false, false)
    NQK_PG_CASE_PC(PG_RESID, 12, true, false, false)
    NQK_PG_CASE_PC(PG_RESID, 12, false, false, false)
    NQK_PG_CASE_PC(PG_RESID, 48, true, false, false)
    NQK_PG_CASE_PC(PG_RESID, 48, false, false, false)
    NQK_PG_CASE_PC(PG_QKV, 3, true, false, true)
    NQK_PG_CASE_PC(PG_QKV, 3, true, false, false)
    NQK_PG_CASE_PC(PG_GELU, 3, true, false, false)
    NQK_PG_CASE_PC(PG_GLUT, 3, true, false, false)
    NQK_PG_CASE_PC(PG_GLUT1, 3, true, false, false)
    NQK_PG_CASE_PC(PG_RESID, 3, true, false, false)
    NQK_PG_CASE_PC(PG_RESID, 3, false, false, false)
    default:
      return false;
  }
}
}  // namespace nqk
