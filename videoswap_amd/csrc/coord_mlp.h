// What the forward (atlas.hip, K13 / K14) and the backward (atlas_bwd.hip, K16) of the coordinate MLP share: the limits,
// the geometry of the packed weight buffer (vsx.h K13) and the option checks, word for word the same in every entry point.
#pragma once
#include "common.h"

namespace {

constexpr int CM_BM = 64;            // rows per workgroup of the forward
constexpr int CM_THREADS = 256;
constexpr int CM_MAX_LAYERS = 8;
constexpr int CM_MAX_ENC = 64;       // encoded input columns (2 * input_dim * pe_dim), padded to a multiple of 8

inline long cm_round_up(long x, long m) { return (x + m - 1) / m * m; }

inline bool cm_has_enc(int l, int64_t skip_mask) { return l == 0 || ((skip_mask >> l) & 1); }

// floats of the packed weight buffer (vsx.h) of a network with `enc` encoded columns, arguments already validated
inline long cm_packed_floats(int64_t enc, int64_t hidden_dim, int64_t mlp_layers, int64_t skip_mask) {
    const long encp = cm_round_up(enc, 8);
    long total = 0;
    for (int l = 0; l < mlp_layers; ++l) {
        const long fp = l == mlp_layers - 1 ? 32 : hidden_dim;
        const long kp = (l > 0 ? hidden_dim : 0) + (cm_has_enc(l, skip_mask) ? encp : 0);
        total += fp * kp + fp;
    }
    return total;
}

// the options of IMLP_Hash that a coordinate network (pe_type none / encoding) can be built with -> *enc, its encoded columns
inline int cm_check_options(const char* what, int64_t mlp_type, int64_t pe_type, int64_t input_dim, int64_t pe_dim, int64_t* enc) {
    VSX_REQUIRE(mlp_type == 0, VSX_E_UNSUPPORTED, "%s: mlp_type 'tcnn' (%lld) is not implemented, only 'origin'", what,
                (long long)mlp_type);
    VSX_REQUIRE(pe_type == 0 || pe_type == 1, VSX_E_UNSUPPORTED,
                "%s: pe_type 'hash_encoding' (%lld) is not implemented, only 'none' and 'encoding'", what, (long long)pe_type);
    VSX_REQUIRE(input_dim == 2 || input_dim == 3, VSX_E_UNSUPPORTED, "%s: input_dim %lld (2 or 3)", what, (long long)input_dim);
    *enc = pe_type == 1 ? 2 * input_dim * pe_dim : input_dim;
    VSX_REQUIRE(pe_type == 0 || (pe_dim >= 1 && *enc <= CM_MAX_ENC), VSX_E_UNSUPPORTED,
                "%s: pe_dim %lld (2 * input_dim * pe_dim must be 1 to %d)", what, (long long)pe_dim, CM_MAX_ENC);
    return VSX_OK;
}

// the layer stack's own limits
inline int cm_check_stack(const char* what, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers, int64_t skip_mask) {
    VSX_REQUIRE(output_dim >= 1 && output_dim <= 3, VSX_E_UNSUPPORTED, "%s: output_dim %lld (1 to 3)", what, (long long)output_dim);
    VSX_REQUIRE(hidden_dim >= 32 && hidden_dim <= 256 && hidden_dim % 32 == 0, VSX_E_UNSUPPORTED,
                "%s: hidden_dim %lld (a multiple of 32 up to 256)", what, (long long)hidden_dim);
    VSX_REQUIRE(mlp_layers >= 2 && mlp_layers <= CM_MAX_LAYERS, VSX_E_UNSUPPORTED, "%s: mlp_layers %lld (2 to 8)", what,
                (long long)mlp_layers);
    VSX_REQUIRE(skip_mask >= 0 && (skip_mask & 1) == 0 && (skip_mask >> mlp_layers) == 0, VSX_E_UNSUPPORTED,
                "%s: skip_layers must lie in 1 .. mlp_layers - 1 (mask 0x%llx)", what, (long long)skip_mask);
    return VSX_OK;
}

// floats of the `saved` buffer of a training forward (vsx.h K16)
inline long cm_saved_floats(long N, int64_t enc, int64_t output_dim, int64_t hidden_dim, int64_t mlp_layers) {
    return N * ((mlp_layers - 1) * hidden_dim + enc + output_dim);
}

}  // namespace
