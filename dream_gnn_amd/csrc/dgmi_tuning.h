// dgmi_tuning.h — the handful of launch parameters the measurement tools override (tools/*.py, one test).
// Read ONCE from the environment (DGMI_*), when the library is first asked for them, and afterwards changed only
// through dgmi_set_tuning (include/dgmi.h): no launch path calls getenv.  0 / -1 = the built-in choice.
#pragma once
#include <stdint.h>

namespace dgmi {

struct Tuning {
  int sliced_rows = 0;              // DGMI_SLICED_ROWS: destination rows per lane group of the XCD-local kernel
  int sliced_touch_lead = -1;       // DGMI_SLICED_PF: worker blocks between a toucher and what it touches (0: no touchers)
  int sliced_lpr = 0;               // DGMI_SLICED_LPR: lane-group width 8 / 16 / 32 / 64
  int sliced_no_off32 = 0;          // DGMI_NO_OFF32: 64-bit row addresses even where 32-bit offsets fit
  int64_t sliced_chunk_rows = 0;    // DGMI_SLICED_CHUNK_ROWS: destination rows per launch pair
  int64_t sliced_taper_rows = 0;    // DGMI_SLICED_TAPER_ROWS: last rows of a chunk in shorter runs (-1: off, 0: built-in)
  int sliced_owned = -1;            // DGMI_SLICED_OWNED: the workgroup-owned form (dgmi_owned.hip) 0 = never, 1 = whenever applicable, -1 = built-in rule
  int sliced_owned_grid = 0;        // DGMI_SLICED_OWNED_GRID: its workgroups (0: one per CU)
  int sliced_owned_wgs = 0;         // DGMI_SLICED_OWNED_WGS: its workgroups per CU (0: built-in, 1: one of 16 waves, 2: two of 12 waves)
  int sliced_owned_rows = 0;       // DGMI_SLICED_OWNED_ROWS: rows per lane group and task (0: built-in)
  int64_t sliced_owned_lds_rows = 0;  // DGMI_SLICED_OWNED_LDS_ROWS: cap on a workgroup's LDS rows (forces row rounds; 0: the LDS budget)
  int sliced_owned_workers = 0;     // DGMI_SLICED_OWNED_WORKERS: worker waves of a workgroup that take tasks, the others leave at once (0: all; 1: one wave runs every task in order; never changes a bit; test)
  int sliced_owned_slices = 0;      // DGMI_SLICED_OWNED_SLICES: slices of the layouts made for the owned form (dgmi_sliced_layout_slices; 0: built-in rule, n: n for every product it can plan — which form then runs on them is still sliced_owned's rule: 1 to run the owned form; a bf16 table, for which no such layout is made, runs the pair while a count is forced)
  int sliced_owned_scaled = -1;    // DGMI_SLICED_OWNED_SCALED: the owned form's scaled kernel (scale codes in the id words, include/dgmi_scale.h) 0 = never, 1 = wherever it is built and the owned form takes the product, -1 = built-in rule (its measured classes; everything it is built for while sliced_owned = 1 forces the form)
  int sliced_owned_duty = -1;      // DGMI_SLICED_OWNED_DUTY: the owned form without a toucher — sixteen workers, the touching a duty of task slots (dgmi_owned_kernel.h) 0 = never, 1 = wherever it is built (an fp32 table, 32-bit offsets, 16- or 32-lane groups, no gate, one workgroup per CU), -1 = built-in rule (its measured classes)
  int sliced_owned_duty_chunk = 0;  // DGMI_SLICED_OWNED_DUTY_CHUNK: task slots per duty (0: built-in, a whole phase)
  int sliced_owned_duty_lead = 0;   // DGMI_SLICED_OWNED_DUTY_LEAD: task slots a duty touches ahead (0: built-in, one chunk)
  int sliced_owned_lag = -2;       // DGMI_SLICED_OWNED_LAG: phases a workgroup may run ahead of its XCD's slowest (-1: no gate, -2: built-in)
  int64_t sliced_owned_spin_ticks = 0;  // DGMI_SLICED_OWNED_SPIN_TICKS: bound of one gate wait, 100 MHz ticks (0: built-in)
  int64_t select_window_min = 0;    // DGMI_SELECT_WINDOW_MIN: shortest list that takes the window passes
  int select_narrow_window = 0;     // DGMI_SELECT_NARROW_WINDOW: a window that misses (forces the take-over path; test)
  int sort_plain_tiles = 0;         // DGMI_SORT_PLAIN_TILES: record sort with tile = blockIdx.x instead of the XCD-aware order
  int knn_screen_first = 0;         // DGMI_KNN_SCREEN_V1: the first (register-staged) 256 x 256 screen kernel instead of the LDS-DMA one (A/B tools)
  int64_t knn_pool_chunks = 0;      // DGMI_KNN_POOL_CHUNKS: chunks of the screen's record pool (a pool that runs out: the direct appends; test)
};

Tuning& tuning();  // dgmi_api.hip

}  // namespace dgmi
