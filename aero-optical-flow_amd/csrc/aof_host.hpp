// Host-only services the host files lend each other, and the alignment test every entry point and launcher makes.
// Structs of other headers appear here by name only: whoever calls a service includes the header of what it passes.
#pragma once

#include <cstddef>
#include <cstdint>

#include "aof.h"

namespace aof {

struct SmallArgs;                            // (aof_engine_args.hpp)
struct FieldGeom;                             // (aof_field_step.hpp)

// Is p a multiple of n bytes (nullptr is)?  The host-side test of every entry point and launcher; kernels test their own.
inline bool aligned(const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

// The rate limiter's period in microseconds, 0 without a limit: the facade's own division, in float.
inline float limiter_period_us(int output_rate) { return output_rate > 0 ? 1.0e6f / (float)output_rate : 0.0f; }

// The motion-field fit's host side (aof_field.cpp), for the stream bank's motion field (aof_bank_field.cpp): are the
// parameters outside their ranges; the geometry of a configuration's level-0 grid, or -EINVAL where the fit does not serve
// it; and the fit of one pair on host memory (flow: read for pred_x / pred_y).
bool field_bad_params(const aof_field_params *fp);
int field_geom(const aof_params *p, const aof_field_params *fp, FieldGeom *out);
void field_pair(const FieldGeom &g, const aof_block *blocks, const uint8_t *subdirs, const aof_flow &flow, aof_field *out);
// (aof_batch.cpp) the small-pair plan of n pairs, whatever n: true where one workgroup per pair can serve the
// context's configuration and these buffers (flows: [n]; d_workspace: aof_workspace_layout(p, n))
bool plan_small_batch(const aof_ctx *ctx, const uint8_t *prev, const uint8_t *cur, int64_t stride, int64_t n, aof_flow *flows,
                      void *d_workspace, SmallArgs *sm);
// (aof_batch.cpp) the small-pair plan of a configuration alone (no context, no buffers: pointers that are only looked at
// for their alignment): true where one workgroup per pair can serve `p`
bool plan_small_params(const aof_params *p, SmallArgs *sm);
// (aof_capi.hip) sticky fault / wedged state and current-device check of a context, before anything is enqueued; and
// aof_last_error's text for the callers outside aof_capi.hip
int precheck(aof_ctx *ctx);
int ctx_fail(aof_ctx *ctx, int code, const char *what);
// (aof_batch.cpp) the flow of a frame sequence for the pipeline: does the call run K1 as a pass of its own, and the
// call itself with K1's outputs already in the workspace
bool sequence_runs_k1(aof_ctx *ctx, const uint8_t *d_frames, int64_t n_pairs, void *d_workspace);
int flow_sequence(aof_ctx *ctx, const uint8_t *d_frames, int64_t n_pairs, aof_flow *d_flows, void *d_workspace,
                  size_t workspace_bytes, void *stream, bool k1_ready);

}  // namespace aof
