// Launcher of the attention-location kernels (attloc.hip): every attention map reduced to a position -- arg-max cell, central-mass box, moments,
// entropy -- and the maps of a row added up over time into its coverage.  include/lxo.h (lxo_attention_locate) holds the definition.
#pragma once
#include "lxo_common.h"

// the most cells a map may have: what one wave stages in LDS (38 KB of f32).  98 x 98 = 9604, the largest bucket's map, fits.
constexpr int kLocateMaxCells = 9728;
constexpr int kLocateStats = 8;

// Position (i, t), i < rows, t < steps: the map at alpha + t step_stride + r row_stride (floats), r = src[t rows + i] (NULL: i), Hp x Wp cells row-major.
// No map -- t >= len[i] (NULL: never), r outside [0, alpha_rows), a sum that is not positive and finite -- gives the "none" values.  peak int32
// [rows][steps], box int32 [rows][steps][4], stats f32 [rows][steps][kLocateStats], coverage f32 [rows][cov_ld] (cells [0, Hp Wp) written); each
// nullable.  One launch of one wave per position for peak / box / stats, one launch for coverage behind it (it reads the first launch's "none"
// marks; with coverage alone it sums the maps itself).  No atomics, no host synchronisation.  Hp Wp > kLocateMaxCells or more waves than a grid
// holds: -2.
struct LocateArgs {
    const float* alpha; const int* len; const int* src;
    int* peak; int* box; float* stats; float* coverage;
    long long step_stride, row_stride;
    int alpha_rows, Hp, Wp, rows, steps, cov_ld;
    float mass;
};
int lxo_k_attention_locate(const LocateArgs& a, hipStream_t st);
