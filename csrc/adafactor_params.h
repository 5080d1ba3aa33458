// Geometry and unit-table layout of the Adafactor kernels (csrc/adafactor.hip), shared with the host code that plans
// the table (csrc/bind_optim.cpp adafactor_plan) so that both sides enumerate the same tiles and scratch offsets.
#pragma once

// A unit (one transformers parameter: a whole flat segment, or one dim-0 slice of a fused one) is cut into tiles of
// AF_RB rows x AF_CC columns; a workgroup of 4 waves takes one tile, wave w the AF_WC columns from w * AF_WC, each lane 4
// of them.  1-D units are one row of `numel` columns.
constexpr int AF_RB = 32;                // rows per tile: the per-lane column-sum chain
constexpr int AF_WC = 256;               // columns per wave
constexpr int AF_CC = 4 * AF_WC;         // columns per tile
constexpr int AF_GRID_CAP = 2048;        // workgroups per tile pass: 256 CUs x 8 resident 256-thread workgroups
constexpr int AF_FIN_SLICES = 16;        // row-block slices summed in parallel per column in the statistics finalize
constexpr int AF_FIN_COLS = 16;          // columns per finalize iteration (AF_FIN_SLICES x AF_FIN_COLS = 256 threads)
constexpr int AF_FIN_Y = 8;              // workgroups per unit in the statistics finalize (column groups strided)

// int64 fields of one unit-table row; the table has one extra row whose AF_TILE0 is the total tile count
enum {
  AF_OFF = 0,      // flat element offset of the unit
  AF_ROWS,         // rows (1 for a 1-D unit)
  AF_COLS,         // columns (numel of a 1-D unit)
  AF_RV,           // offset of R[rows] (factored) or V[numel] (1-D) in the row/vector state buffer
  AF_C,            // offset of C[cols] in the column state buffer, -1 for a 1-D unit
  AF_DECAY,        // 1 where weight decay applies
  AF_TILE0,        // first tile of the unit (prefix sum of tile counts)
  AF_COLPART,      // offset of the unit's [row blocks, cols] column partial sums
  AF_ROWPART,      // offset of the unit's [rows, column chunks] row partial sums
  AF_NCHUNK,       // column chunks per row: ceil(cols / AF_CC)
  AF_VEC,          // 1: 16-byte access (cols % 4 == 0 and every offset % 4 == 0), 0: scalar path
  AF_SCAL,         // index of the unit's row in the per-unit scalar array [units, 4]
  AF_FIELDS
};
