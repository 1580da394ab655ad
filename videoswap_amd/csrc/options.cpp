// The option table of the whole library: vsx_set_option, vsx_get_option and vsxg::gemm_option (options.h).  An option's initial value
// comes from its environment variable the first time it is asked for; vsx_set_option overrides it.  Every option is for A/B runs and tests: the
// product path runs on the defaults.
//
//   name          environment       default  meaning
//   gemm_pp       VSX_GEMM_PP       1        persistent ping-pong GEMM (gemm_pp.hip): 0 = never, 1 = where it is expected to win (the
//                                            thresholds of plan_gemm, gemm.hip), 2 = 256-row tiles wherever >= 64 of them exist, else
//                                            128-row tiles from 32, 3 = 128-row tiles wherever >= 32 exist, 4 = 256-row tiles for every
//                                            eligible problem however small (tools/cpu_check)
//   pp_sched      VSX_PP_SCHED      0        schedule bits (gemm_common.h: PP_* / TILE_RES_EARLY): 4 = tap-major convolution K order,
//                                            8 = linear tile walk, 16 = a private A slab per convolution tap, 32 = every CU issues the
//                                            pieces of a slab in the common order, 64 = tile kernels prefetch the residual in front of
//                                            the K loop
//   tile_tune     VSX_TUNE_TILE     0        tile + 16 * deep + 256 * splits (gemm.hip): tile 1|2|3 forces the 128x320 / 128x160 /
//                                            256x320 tile kernel where the column count is a multiple of 320, 4|5|6 the 128x128 /
//                                            64x128 / 64x64 tile for any; deep = four ring slots for the 128x160 tile; splits > 0 = that
//                                            many K slices where split-K is possible at all
//   xcd_walk      VSX_XCD_WALK      1        tile kernels: 1 = XCD block grid where it moves fewer bytes (gemm.hip: plan_xcd_grid),
//                                            0 = the linear walk
//   attn_qb       VSX_ATTN_QB       0        flash attention at d = 40 / 80: 0 = the rule of launch_attn (attention.hip), 1 / 2 = always
//                                            that many 32-query blocks per wave
//   temporal_out  VSX_TEMPORAL_OUT  0        1 = temporal attention stores from the accumulator layout instead of through LDS
//   attn_o16      VSX_ATTN_O16      0        1 = flash attention at d = 40 with O^T on 16x16x32 MFMA tiles (measured neutral)
//   gn_fuse       VSX_GN_FUSE       0        1 = GroupNorm statistics finalized in the apply kernel's prologue where an image has at most
//                                            64 chunks (measured 2 % slower)
//   gemm_ws       VSX_GEMM_WS       1        weight-stationary K = 320 GEMM (gemm_pp.hip: gemm_ws320_kernel): 0 = never, 1 = K = N = 320
//                                            with a residual from 65 536 rows, 2 = every eligible problem (tests), 3 = as 1 from 131 072
//                                            rows, 4 = 1 + the LayerNorm-folded 320 -> 640 / 960 projections, 5 = 1 + the residual-free
//                                            K = N = 320 launches from 131 072 rows
//   ws_waves      VSX_WS_WAVES      10       weight-stationary kernel: 10 waves of 32 columns or 5 waves of 64 (= row-statistics parts per
//                                            320 columns)
//   conv_winograd VSX_CONV_WINOGRAD 1        Winograd F(2x2, 3x3) form of the stride-1 3x3 convolutions (winograd.hip): 0 = never, 1 = the
//                                            shapes of vsx_conv3x3_winograd_auto unless a GEMM back end is forced (gemm_pp != 1 or
//                                            tile_tune != 0), 2 = every supported description (tests).  That function is the one
//                                            statement of the rule: ops.conv2d asks it for every stride-1 3x3 convolution
#include "options.h"

#include <stdlib.h>
#include <string.h>

#include "common.h"

namespace vsxg {
namespace {
struct Option { const char* name; const char* env; long value; bool init; };
Option g_options[] = {{"gemm_pp", "VSX_GEMM_PP", 1, false}, {"pp_sched", "VSX_PP_SCHED", 0, false},
                      {"tile_tune", "VSX_TUNE_TILE", 0, false}, {"xcd_walk", "VSX_XCD_WALK", 1, false},
                      {"attn_qb", "VSX_ATTN_QB", 0, false}, {"temporal_out", "VSX_TEMPORAL_OUT", 0, false},
                      {"attn_o16", "VSX_ATTN_O16", 0, false}, {"gn_fuse", "VSX_GN_FUSE", 0, false},
                      {"gemm_ws", "VSX_GEMM_WS", 1, false}, {"ws_waves", "VSX_WS_WAVES", 10, false},
                      {"conv_winograd", "VSX_CONV_WINOGRAD", 1, false}};
Option* find_option(const char* name) {
    for (auto& o : g_options)
        if (strcmp(o.name, name) == 0) {
            if (!o.init) {
                const char* e = getenv(o.env);
                if (e) o.value = atol(e);
                o.init = true;
            }
            return &o;
        }
    return nullptr;
}
}  // namespace
long gemm_option(const char* name) {
    Option* o = find_option(name);
    return o ? o->value : 0;
}
}  // namespace vsxg

extern "C" int vsx_set_option(const char* name, int64_t value) {
    auto* o = name ? vsxg::find_option(name) : nullptr;
    if (!o) return vsx_fail(VSX_E_BADSHAPE, "vsx_set_option: unknown option '%s'", name ? name : "(null)");
    o->value = (long)value;
    return VSX_OK;
}

extern "C" int vsx_get_option(const char* name, int64_t* value) {
    auto* o = name ? vsxg::find_option(name) : nullptr;
    if (!o) return vsx_fail(VSX_E_BADSHAPE, "vsx_get_option: unknown option '%s'", name ? name : "(null)");
    VSX_REQUIRE(value != nullptr, VSX_E_BADSHAPE, "vsx_get_option: null value pointer");
    *value = o->value;
    return VSX_OK;
}
