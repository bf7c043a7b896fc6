// obmc_row_eighth.hip -- the row formulation of OBMC (obmc_row_body.h, RK 3) at eighth pel: the four taps of the tiled
// half-pel images blended with orc_combine4_nxm_u8's general weights (schroframe.c:2288-2413,
// schroorc.orc:1635-1662) on pairs of 16-bit sums.

#include "obmc_row_body.h"

namespace schro {
namespace {

SCHRO_ROW_KERNEL (obmc_row_eighth_2_1, 6, 2, 1, false, kRTH, false, 3)
SCHRO_ROW_KERNEL (obmc_row_eighth_3_1, 6, 3, 1, false, kRTH, false, 3)
SCHRO_ROW_KERNEL (obmc_row_eighth_4_1, 5, 4, 1, false, kRTH, false, 3)
SCHRO_ROW_KERNEL (obmc_row_eighth_uv_2, 5, 2, 1, true, kRTH, false, 3)
SCHRO_ROW_KERNEL (obmc_row_eighth_uv_3, 6, 3, 1, true, kRTH, false, 3)
SCHRO_ROW_KERNEL (obmc_row_eighth_uv_4, 5, 4, 1, true, kRTH, false, 3)
SCHRO_ROW_KERNEL (obmc_row_eighth_p_3_1, 7, 3, 1, false, kRTH, true, 3)
SCHRO_ROW_KERNEL (obmc_row_eighth_p_uv_3, 7, 3, 1, true, kRTH, true, 3)
SCHRO_ROW_KERNEL (obmc_row_eighth_h2_3_1, 6, 3, 1, false, kRTH, false, 3, 2)
SCHRO_ROW_KERNEL (obmc_row_eighth_h2_uv_3, 6, 3, 1, true, kRTH, false, 3, 2)
SCHRO_ROW_KERNEL (obmc_row_eighth_h2_4_1, 5, 4, 1, false, kRTH, false, 3, 2)
SCHRO_ROW_KERNEL (obmc_row_eighth_h2_uv_4, 5, 4, 1, true, kRTH, false, 3, 2)

// picture weights other than 1, 1 / 2 (fades)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_3_1, 6, 3, 1, false, kRTH, false, 3, 1, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_uv_3, 6, 3, 1, true, kRTH, false, 3, 1, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_p_3_1, 6, 3, 1, false, kRTH, true, 3, 1, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_p_uv_3, 6, 3, 1, true, kRTH, true, 3, 1, true)
// ... and one kernel per other form (it serves the prediction-only launches of its form too)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_2_1, 5, 2, 1, false, kRTH, false, 3, 1, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_4_1, 5, 4, 1, false, kRTH, false, 3, 1, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_uv_2, 5, 2, 1, true, kRTH, false, 3, 1, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_uv_4, 5, 4, 1, true, kRTH, false, 3, 1, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_h2_3_1, 6, 3, 1, false, kRTH, false, 3, 2, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_h2_uv_3, 6, 3, 1, true, kRTH, false, 3, 2, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_h2_4_1, 5, 4, 1, false, kRTH, false, 3, 2, true)
SCHRO_ROW_KERNEL (obmc_row_eighth_w_h2_uv_4, 5, 4, 1, true, kRTH, false, 3, 2, true)

constexpr RowEntry kEighth[] = {
  ROW_ENTRY (obmc_row_eighth_2_1), ROW_ENTRY (obmc_row_eighth_3_1), ROW_ENTRY (obmc_row_eighth_4_1), ROW_ENTRY (obmc_row_eighth_uv_2),
  ROW_ENTRY (obmc_row_eighth_uv_3), ROW_ENTRY (obmc_row_eighth_uv_4), ROW_ENTRY (obmc_row_eighth_p_3_1), ROW_ENTRY (obmc_row_eighth_p_uv_3),
  ROW_ENTRY (obmc_row_eighth_h2_3_1), ROW_ENTRY (obmc_row_eighth_h2_uv_3), ROW_ENTRY (obmc_row_eighth_h2_4_1), ROW_ENTRY (obmc_row_eighth_h2_uv_4),
  ROW_ENTRY (obmc_row_eighth_w_3_1), ROW_ENTRY (obmc_row_eighth_w_uv_3), ROW_ENTRY (obmc_row_eighth_w_p_3_1), ROW_ENTRY (obmc_row_eighth_w_p_uv_3),
  ROW_ENTRY (obmc_row_eighth_w_2_1), ROW_ENTRY (obmc_row_eighth_w_4_1), ROW_ENTRY (obmc_row_eighth_w_uv_2), ROW_ENTRY (obmc_row_eighth_w_uv_4),
  ROW_ENTRY (obmc_row_eighth_w_h2_3_1), ROW_ENTRY (obmc_row_eighth_w_h2_uv_3), ROW_ENTRY (obmc_row_eighth_w_h2_4_1),
  ROW_ENTRY (obmc_row_eighth_w_h2_uv_4),
};
constexpr RowTable kEighthTable = { kEighth, (int) std::size (kEighth) };
static_assert (row_table_ok (kEighthTable, 3), "obmc_row_eighth.hip: one kernel per form");
static_assert (row_find (kEighthTable, RowForm { 3, 2, 1, 1, true, false }) == obmc_row_eighth_2_1, "obmc_row_eighth.hip: a prediction_only launch without a kernel of its form takes the residual form's");

}                               // namespace

RowTable
obmc_row_table_eighth ()
{
  return kEighthTable;
}

}                               // namespace schro
