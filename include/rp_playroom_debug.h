/* rp_playroom_debug.h — test / tuning hooks exported by librp_playroom_hip.so next to the C ABI of rp_playroom.h.
 *
 * Nothing here stands in for a reference interface: these exist so that the parity tests can compare the library's two step
 * pipelines with each other and with the oracle at intermediate points, and so that profiling scripts can pin the launch
 * layout.  None of them changes a result (both pipelines and every group / slot layout are bit-identical; tests/ check it).
 * tests/test_abi.py checks that every rp_* symbol the library exports is declared in one of the two headers. */
#ifndef RP_PLAYROOM_DEBUG_H
#define RP_PLAYROOM_DEBUG_H
#include "rp_playroom.h"

#ifdef __cplusplus
extern "C" {
#endif

/* step pipeline: 0 = split kernels (default), 1 = one fused kernel per env step (k_step; the in-library cross-check), 2 = the twelve substeps of a step in one launch
 * (k_chain, round 4's experiment: blocks of two waves own four envs for the whole step; grid = RP_CHAIN_BLOCKS read at rp_create, default 1024).  All three produce the
 * same bits (tests/).  With fused = 1 and timers enabled rp_step synchronises on its own kernel to read the timer; fused = 2 has no per-launch timers: rp_set_fused(h, 2)
 * with timers on, and rp_enable_timers(h, n > 0) under fused = 2, return RP_ERR_ARG. */
int rp_set_fused(rp_handle h, int32_t fused);
/* number of env groups (streams) of the split pipeline, 1 .. 16 */
int rp_set_groups(rp_handle h, int32_t groups);
/* bit 0: the solver gives every contact its own folded slot (its fallback layout) instead of solving arm-only and non-arm
 * contacts side by side */
int rp_set_debug_flags(rp_handle h, int32_t flags);
/* one fused substep on every env on the NULL stream; intermediates of env `env` into host_buf[4096] (layout: k_debug_substep) */
int rp_debug_substep(rp_handle h, int32_t env, float* host_buf);
/* per env of the most recent k_prep2: host_buf[2 e] = unit rows, host_buf[2 e + 1] = contacts + 1000 * (arm contact) + 100000 *
 * spanning contacts; synchronises the device */
int rp_debug_row_counts(rp_handle h, int32_t* host_buf);
/* the joints [num_envs][8] of the ghost arm(s) drawn by the latest rp_render_ex with a ghost_arm (environments.py:575-590: rest pose, one IK call, joints [0:6]) */
int rp_debug_ghost_joints(rp_handle h, float* host_buf, int32_t num_envs);
/* the render kernel's tile shortlist (rp_render, rp_render_ex and rp_render_layers alike: one kernel draws for all three): on = 1 (the default) a tile walks only the
 * records whose bounding sphere meets its frustum; on = 0 every record is on every tile's list.  The layers are bit-identical either way (tests/test_gpu_render_layers.py); tools/render_rate.py times one against the other. */
int rp_debug_render_cull(rp_handle h, int32_t on);
/* the image passes of rp_set_image_views with two or more views: on = 1 (the default) one k_render_views launch draws the tiles of all views of a pass; on = 0 one
 * k_render_layers launch per view, behind the same single k_collider_poses.  The layers are bit-identical either way (tests/test_gpu_image_views.py);
 * tools/image_views_rate.py times one against the other. */
int rp_debug_image_views_merge(rp_handle h, int32_t on);
/* rp_render_states' chunks: at most `slots` images per chunk (0, the default: the rule of rp_playroom.h, min(m, max(N, 4096))), so that a test crosses chunk
 * boundaries with seven images instead of 4097.  The images are bit-identical whatever the chunk size (tests/test_gpu_render_states.py).  rp_closest_points walks
 * its rows in the same chunks and obeys the same cap (tests/test_gpu_closest_points.py).  RP_ERR_ARG: slots < 0. */
int rp_debug_render_states_chunk(rp_handle h, int32_t slots);
/* rounds the most recent rp_reset took */
int rp_debug_reset_rounds(rp_handle h);
/* k_autoreset's launch shape, fixed at rp_create: *grid = its blocks (the blocks resident at once, or RP_AUTORESET_BLOCKS; never more than
 * ceil(num_envs / epb)), *epb = the envs a block settles side by side (RP_AUTORESET_EPB, 1 .. 4) */
int rp_debug_autoreset_shape(rp_handle h, int32_t* grid, int32_t* epb);
/* the action stage alone (clip, action type, IK, clamps, motor targets: k_action's body, 64-thread blocks, 16 lanes per env) on the current state, NULL stream, synchronised.
 * Blocks are cut by the latest step's member table and group bounds as they stand (the next step would re-rank first); before the first step of a pipeline, in identity
 * order with rp_set_groups' groups.  action_dev [N][dims.action] (unclipped, as rp_step takes it); raw_dev [N][8] floats: the joint solution BEFORE the clamps to the joint
 * limits and to q +- inc (7, zero-padded), then 1 * capped + 2 * marginal + 4 * place - the conditions behind status bits 8 and 16, and the env's place in the member table
 * (place / 4 within its group's launch is its block, place % 4 its DPP row).  As in a step the motor targets and the status word are written into the state; nothing else is. */
int rp_debug_action(rp_handle h, const float* action_dev, float* raw_dev);
/* PROFILING BUILDS ONLY (tools/build_profiling_libs.sh: -DRP_CLOCKS=1|2, -DRP_PROLOGUE_CLOCKS, -DRP_CHAIN_CLOCKS).  The shipped library exports none of these and
 * tests/test_abi.py does not expect them; such a build also exports, for the tools that load it through RP_PLAYROOM_LIB:
 *     rp_debug_clocks(rp_handle, uint64_t* host_buf, int32_t nwaves)              s_memtime marks per wave of k_solve2 (RP_CLOCKS=1) / per block of k_prep2 (=2)
 *     rp_debug_prologue_clocks(rp_handle, uint64_t* host_buf, int32_t nwaves)     marks of k_solve2's prologue
 *     rp_debug_chain_clocks(rp_handle, int64_t* host_buf, int32_t nblocks)        per block of k_chain: prepare / solve totals
 * each copies the marks of the most recent launch to the host after a device synchronise. */

#ifdef __cplusplus
}
#endif
#endif
