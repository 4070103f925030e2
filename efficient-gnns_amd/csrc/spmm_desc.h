// Host-side argument checks of the egnn_spmm_t descriptor (include/egnn_hip.h), shared by the launchers of spmm.hip and spmm_blk.hip.
#pragma once
#include "common.h"

// the parts of the descriptor an entry point reads beyond n_rows / K / rowptr / index_bits / bias / Y / ldy / reduce
constexpr unsigned kSpmmGather = 1;     // n_src, col, val, src_scale, X, ldx (everything but the combine step)
constexpr unsigned kSpmmEpilogue = 2;   // addend, ld_addend, stat_part, stat_shift, flags (block schedule + combine step)

// The EGNN_EINVAL checks that come before the "nothing to do" return of every entry point: sizes, index width, reduce, and -- on the
// schedules without an epilogue -- that none is asked for.  Pointers and alignment are checked by the entry point itself, after it.
static inline int spmm_check(const egnn_spmm_t* op, unsigned parts, bool max_ok = false) {
  EGNN_CHECK_ARG(op && op->n_rows >= 0 && op->K >= 0 && op->ldy >= op->K);
  EGNN_CHECK_ARG(!(parts & kSpmmGather) || (op->n_src >= 0 && op->ldx >= op->K));
  EGNN_CHECK_ARG(op->index_bits == 32 || op->index_bits == 64);
  EGNN_CHECK_ARG(op->reduce == EGNN_SUM || op->reduce == EGNN_MEAN || (max_ok && op->reduce == EGNN_MAX));
  EGNN_CHECK_ARG((parts & kSpmmEpilogue) || (!op->addend && !op->stat_part && !(op->flags & 8)));
  return EGNN_OK;
}
