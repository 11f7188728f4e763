// dcx_cell_dev.h -- the packed code of one 8x8 cell, loc | id << 8 (loc: arg-max of the 65 location classes, id: arg-max of the
// n_ids + 1 id classes after the dust-bin rule), as dcx_misc.hip's decode kernels and dcx_tail.hip's fused tail write and read it.
#pragma once
#include "dcx_common.h"

__device__ __forceinline__ int dcx_cell_pack(int la, int ia) { return la | (ia << 8); }
__device__ __forceinline__ int dcx_cell_loc(int code) { return code & 255; }
__device__ __forceinline__ int dcx_cell_id(int code) { return code >> 8; }
// where(loc_argmax == 64, dust_bin, ids_argmax)  model_utils.py:76; no_corner = the last location class
__device__ __forceinline__ int dcx_cell_masked_id(int la, int no_corner, int ia, int dust_bin) { return la == no_corner ? dust_bin : ia; }
// mask = ids != dust_bin_ids  model_utils.py:111
__device__ __forceinline__ bool dcx_cell_fires(int code, int dust_bin) { return dcx_cell_id(code) != dust_bin; }
// the row (x, y, id, cell) of a firing cell of a map wc cells wide: xs = 8*ix + loc % 8, ys = 8*iy + loc // 8  (model_utils.py:121-122)
__device__ __forceinline__ int4 dcx_cell_row(int code, int cell, int wc) {
    const int la = dcx_cell_loc(code);
    const int cy = cell / wc, cx = cell - cy * wc;
    return make_int4(8 * cx + (la & 7), 8 * cy + (la >> 3), dcx_cell_id(code), cell);
}
