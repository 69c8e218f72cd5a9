// What the translation units of the un-fused inner loop share beside the arithmetic of rows_stack.h: rows.hip (the row passes),
// slabprox.hip (the slab-coupled proxes; its L2 ball ends in a row pass) and pf2polar.hip (the PARAFAC2 polar factors).
#pragma once
#include "mcl_internal.h"
#include "rows_stack.h"

static __device__ __forceinline__ double wave_sum_d(double v) { return wave_sum(v); }  // DPP + readlane (rows_mfma.h)

// Used for all three modes: A and C are treated as a single slab (tile maps tilesA / tilesC, extents ext_A / ext_C).
static inline ModeView view_of(mcl_context *c, int mode) {
    ModeView v{};
    v.gate = c->gate_active;
    const TileMap &tm = mcl_tiles(c, mode);
    v.tile_slab = tm.slab, v.tile_row0 = tm.row0, v.tile_nrows = tm.nrows, v.n_tiles = tm.n_tiles;
    if (mode == 1) {
        v.ext = c->row_ptr_dev, v.n_slabs = (int)c->I, v.rho = c->rhoB, v.F = c->B;
    } else if (mode == 2) {
        v.ext = c->ext_C, v.n_slabs = 1, v.rho = c->rhoC, v.F = c->C;
    } else {
        v.ext = c->ext_A, v.n_slabs = 1, v.rho = c->rho_max + 1, v.F = c->A;  // constant rho only
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------
// All row kernels use the tile / fragment layout of rows_mfma.h (coalesced 16-B accesses); products with a
// wave-uniform r x r matrix (L^-1, Delta, T_i) run on the fp32 MFMA.
// ---------------------------------------------------------------------------------------------------------
#define FOR_ROW_BLOCKS()                                                                                     \
    _Pragma("unroll") for (int rb = 0; rb < 4; ++rb)                                                         \
        if (16 * rb < nrows)

// launch of a <NBR, VEC> row kernel: one wave per tile, four tiles per workgroup
#define DISPATCH_ROWS(c, vec, KERNEL, grid, block, ...)                                                       \
    do {                                                                                                      \
        const int nbr_ = (c)->r <= 16 ? 1 : ((c)->r <= 32 ? 2 : 4);                                           \
        if (vec) {                                                                                            \
            if (nbr_ == 1) hipLaunchKernelGGL((KERNEL<1, true>), grid, block, 0, (c)->stream, __VA_ARGS__);   \
            else if (nbr_ == 2) hipLaunchKernelGGL((KERNEL<2, true>), grid, block, 0, (c)->stream, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<4, true>), grid, block, 0, (c)->stream, __VA_ARGS__);             \
        } else {                                                                                              \
            if (nbr_ == 1) hipLaunchKernelGGL((KERNEL<1, false>), grid, block, 0, (c)->stream, __VA_ARGS__);  \
            else if (nbr_ == 2) hipLaunchKernelGGL((KERNEL<2, false>), grid, block, 0, (c)->stream, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<4, false>), grid, block, 0, (c)->stream, __VA_ARGS__);            \
        }                                                                                                     \
    } while (0)
