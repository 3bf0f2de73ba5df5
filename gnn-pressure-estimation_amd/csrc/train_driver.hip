// One reference training iteration (train.py:159-190) as a native launch sequence:
// mask -> x[mask]=0 -> forward -> loss on masked nodes (MSE, MAE or SCE) -> backward -> Adam.  See gatres_train_step_t.
#include "gatres_common.h"
#include "gatres_layout.h"
#include "k_update.h"

// GATRES_FLAG_MASK_NEXT with everything the sampling tail of an update launch needs: the step asks for its successor's mask
static bool wants_mask_next(const gatres_train_step_t* ts) {
  return (ts->flags & GATRES_FLAG_MASK_NEXT) && ts->node_ptr && ts->num_graphs > 0 && ts->mask_next && ts->mask_next != ts->mask;
}

// What the step's update launch is given.  wt: the fused path's transposed conv weights, drop_count: where dropped steps
// are counted (either may be null); sample_ahead: the launch also samples the next step's mask.
static UpdateArgs update_args(const gatres_train_step_t* ts, float* wt, uint32_t* drop_count, bool sample_ahead) {
  UpdateArgs u = update_args_of(ts->params, ts->grads, ts->exp_avg, ts->exp_avg_sq, ts->step_counter,
                                gatres_param_count(ts->model.num_blocks, ts->model.nc), ts->lr, ts->beta1, ts->beta2, ts->eps,
                                ts->weight_decay, ts->hparams, ts->grad_scale);
  if (wt) { u.wt = wt; u.nb = ts->model.num_blocks; u.nc = ts->model.nc; }
  u.drop_count = drop_count;
  if (sample_ahead) {
    u.mask_node_ptr = ts->node_ptr; u.mask_graphs = ts->num_graphs; u.mask_rate = ts->mask_rate; u.mask_seed = ts->seed;
    u.mask_next = ts->mask_next;
  }
  return u;
}

// The clipped update of a complete gradient (per-op path, data-parallel Adam phase): norm launch + update launch
static int autoclip_update(const gatres_train_step_t* ts, const UpdateArgs& u, void* stream) {
  int32_t np = 0;
  const int rc = gatres_autoclip_norm_ex(u, ts->autoclip, &np, stream);
  return rc ? rc : gatres_autoclip_update_ex(u, ts->autoclip, np, stream);
}

// Parameter gradients, slab sum and (optionally) Adam of the fused path: the parameter-gradient launch followed by
// gatres_fused_finish.  (The one-launch form, gatres_fused_param_grads_finish, is slower on a single GPU -- 53 us against 38 +
// 9 inside the captured step, k_fused_host.hip -- and serves the data-parallel step's gradient buckets only.)
static int fused_grads_and_update(const gatres_train_step_t* ts, float* wt, const float* loss_part, bool adam, void* stream) {
  // (the step count / fault snapshot: for this call's own update launch, or -- GATRES_FLAG_MASK_NEXT without the Adam phase:
  //  the data-parallel step -- for the sampling tail of the Adam phase that follows the all-reduce)
  const bool snap_later = !adam && (ts->flags & GATRES_FLAG_MASK_NEXT) && ts->step_counter;
  const int rc = gatres_fused_param_grads_ex(&ts->model, ts->graph, ts->saved, ts->scratch,
                                             (adam || snap_later) ? ts->step_counter : nullptr, stream);
  if (rc < 0 || rc > 1) return rc;
  // (rc == 1: the launch left the step count / fault word snapshot the sampling tail of the update launch reads; models whose
  //  parameter gradients do not fold (nc 4 / 8: param_grads_kernel) leave none -- no sampling ahead: the caller finds
  //  mask_next untouched... so it must not rely on it: GATResTrainer asks gatres_fused_finish_folds first)
  const UpdateArgs u = update_args(ts, wt, nullptr, adam && wants_mask_next(ts) && rc == 1);
  float* loss = loss_part ? ts->loss : nullptr;
  if (adam && ts->autoclip) {      // the slab sum leaves the norm partials; the update launch clips, applies Adam, samples ahead
    int32_t np = 0;
    const int rc2 = gatres_fused_finish_norm_ex(&ts->model, ts->graph, ts->scratch, ts->grads, loss_part, loss, u, ts->autoclip,
                                                &np, stream);
    return rc2 ? rc2 : gatres_autoclip_update_ex(u, ts->autoclip, np, stream);
  }
  return gatres_fused_finish_ex(&ts->model, ts->graph, ts->scratch, ts->grads, loss_part, loss, adam ? 1 : 0, u,
                                rc == 1 ? 1 : 0, stream);
}

extern "C" int gatres_train_step(const gatres_train_step_t* ts, void* stream) {
  if (!ts || !ts->graph || !ts->params || !ts->x || !ts->y || !ts->mask || !ts->out || !ts->g_out || !ts->loss ||
      !ts->saved || !ts->scratch)
    return GATRES_E_BADARG;
  const int N = ts->graph->num_nodes;
  int rc = 0;
  // the criterion (GATRES_FLAG_LOSS_*): formed where the forward phase forms the loss -- the window / whole-segment launch
  // (a qualifier of GATRES_PHASE_LOSS) or gatres_masked_loss; the later phases only read the gradient it leaves in g_out
  // and the loss partials it leaves in scratch
  const int32_t crit_flags = ts->flags & (GATRES_FLAG_LOSS_MAE | GATRES_FLAG_LOSS_SCE);
  if (crit_flags == (GATRES_FLAG_LOSS_MAE | GATRES_FLAG_LOSS_SCE)) return GATRES_E_BADARG;
  const int32_t crit = crit_flags == GATRES_FLAG_LOSS_MAE ? GATRES_LOSS_MAE
                       : crit_flags == GATRES_FLAG_LOSS_SCE ? GATRES_LOSS_SCE : GATRES_LOSS_MSE;
  const int32_t loss_phase = GATRES_PHASE_LOSS | (crit == GATRES_LOSS_MAE ? GATRES_PHASE_LOSS_MAE : 0) |
                             (crit == GATRES_LOSS_SCE ? GATRES_PHASE_LOSS_SCE : 0);
  const bool fused = !(ts->flags & GATRES_FLAG_PER_OP) && gatres_fused_supported(&ts->model, ts->graph);
  // GATRES_FLAG_MASK_NEXT can only be honoured where the parameter gradients fold (gatres_fused_finish_folds: their launch
  // leaves the step count / fault snapshot the sampling tail reads).  Refused BEFORE anything is enqueued: a caller that asked for the next
  // mask and did not get it would train on a stale one without noticing.
  if (fused && wants_mask_next(ts) && (ts->phases & GATRES_PHASE_ADAM) && (ts->phases & GATRES_PHASE_BACKWARD) &&
      !gatres_fused_finish_folds(&ts->model, ts->graph))
    return GATRES_E_UNSUPPORTED;
  if (ts->autoclip && (ts->phases & GATRES_PHASE_ADAM)) {      // (refused before anything is enqueued)
    const gatres_autoclip_t* ac = ts->autoclip;
    if (!ac->log || !ac->sorted[0] || !ac->sorted[1] || !ac->ctl || !ac->partials || !ac->norm_out || !ac->clip_out ||
        !ac->coef_out || ac->capacity <= 0 || ac->partials_cap < gatres_autoclip_partials(gatres_param_count(ts->model.num_blocks, ts->model.nc)) ||
        !(ac->percentile >= 0.0 && ac->percentile <= 100.0))
      return GATRES_E_BADARG;
  }
  if ((ts->phases & GATRES_PHASE_MASK) && ts->node_ptr) {
    rc = gatres_mask_generate(ts->node_ptr, ts->num_graphs, ts->mask_rate, ts->seed, ts->step_counter, ts->mask,
                              stream);
    if (rc) return rc;
  }
  if (fused) {
    Layout L;
    if (!make_layout_g(&ts->model, ts->graph, &L)) return GATRES_E_UNSUPPORTED;
    float* loss_part = ts->scratch + L.sc_loss_part;
    float* wt = ts->scratch + L.sc_wt;
    const bool fwd = ts->phases & GATRES_PHASE_FORWARD, bwd = ts->phases & GATRES_PHASE_BACKWARD;
    const bool adam = ts->phases & GATRES_PHASE_ADAM;
    if ((bwd && !ts->grads) || (adam && (!ts->grads || !ts->exp_avg || !ts->exp_avg_sq || !ts->step_counter)))
      return GATRES_E_BADARG;
    // GATRES_FLAG_GRADS_DEFERRED: the backward phase stops after the chain (the kept g_h tables are in scratch); the caller
    // turns them into gradients itself, range by range (gatres_fused_param_grads_finish) -- the data-parallel step starts a
    // bucket's all-reduce between two such launches.
    const bool deferred = (ts->flags & GATRES_FLAG_GRADS_DEFERRED) != 0;
    if (ts->flags & GATRES_FLAG_GRADS_ONLY) {      // (reads the kept tables only: no transposed weights, nothing to prepare)
      if (!bwd || fwd || adam) return GATRES_E_BADARG;
      const bool top = ts->block_hi == ts->model.num_blocks;             // (the launch that also writes the loss)
      return gatres_fused_param_grads_finish(&ts->model, ts->graph, ts->saved, ts->scratch, ts->grads,
                                             top ? loss_part : nullptr, top ? ts->loss : nullptr, 0, nullptr, nullptr,
                                             nullptr, nullptr, 0., 0., 0., 0., 0., nullptr, 1.f, ts->block_lo, ts->block_hi,
                                             stream);
    }
    if (bwd && !(ts->flags & GATRES_FLAG_WT_VALID)) {      // (the fused Adam pass keeps scratch's W^T current)
      rc = gatres_fused_prepare_backward(&ts->model, ts->graph, ts->params, ts->scratch, stream);
      if (rc) return rc;
    }
    if (fwd && bwd) {
      rc = gatres_fused_run(&ts->model, ts->graph, ts->params, ts->x, ts->mask, ts->y, ts->out, ts->g_out, loss_part,
                            nullptr, ts->saved, ts->scratch,
                            GATRES_PHASE_FORWARD | loss_phase | GATRES_PHASE_BACKWARD, stream);
      if (rc || deferred) return rc;
      return fused_grads_and_update(ts, wt, loss_part, adam, stream);
    }
    if (fwd) {
      rc = gatres_fused_run(&ts->model, ts->graph, ts->params, ts->x, ts->mask, nullptr, ts->out, nullptr, nullptr,
                            nullptr, ts->saved, ts->scratch, GATRES_PHASE_FORWARD, stream);
      if (rc) return rc;
      rc = gatres_masked_loss(ts->out, ts->y, ts->mask, crit, ts->loss, ts->g_out, N, stream);
      if (rc) return rc;
    }
    if (bwd) {
      rc = gatres_fused_run(&ts->model, ts->graph, ts->params, ts->x, ts->mask, nullptr, nullptr, ts->g_out, nullptr,
                            nullptr, ts->saved, ts->scratch, GATRES_PHASE_BACKWARD, stream);
      if (rc || deferred) return rc;
      return fused_grads_and_update(ts, wt, nullptr, adam, stream);
    }
    if (adam) {      // (the Adam-only phase of the data-parallel step: keeps scratch's transposed conv weights current too;
                     //  a step whose all-reduced gradient carries a fault mark is dropped and counted in the status block;
                     //  GATRES_FLAG_MASK_NEXT: its extra workgroups sample the next step's mask, from the snapshot the
                     //  parameter-gradient launch of this step left there)
      uint32_t* status = fused_status(ts->scratch, L);
      const bool next = wants_mask_next(ts);
      if (next && !gatres_fused_finish_folds(&ts->model, ts->graph)) return GATRES_E_UNSUPPORTED;      // (no snapshot was left)
      UpdateArgs u = update_args(ts, wt, status + FUSED_STATUS_DROPPED_STEPS, next);
      u.mask_snap = fused_status_snapshot(status);
      return ts->autoclip ? autoclip_update(ts, u, stream) : gatres_adam_step_ex(u, stream);
    }
    return 0;
  }
  if (ts->phases & GATRES_PHASE_FORWARD) {
    rc = gatres_model_forward_per_op(&ts->model, ts->graph, ts->params, ts->x, ts->mask, ts->out, ts->saved, ts->scratch,
                              stream);
    if (rc) return rc;
    rc = gatres_masked_loss(ts->out, ts->y, ts->mask, crit, ts->loss, ts->g_out, N, stream);
    if (rc) return rc;
  }
  if (ts->phases & GATRES_PHASE_BACKWARD) {
    if (!ts->grads) return GATRES_E_BADARG;
    rc = gatres_model_backward_per_op(&ts->model, ts->graph, ts->params, ts->x, ts->mask, ts->g_out, ts->saved, ts->scratch,
                               ts->grads, nullptr, stream);
    if (rc) return rc;
  }
  if (ts->phases & GATRES_PHASE_ADAM) {
    if (!ts->grads || !ts->exp_avg || !ts->exp_avg_sq || !ts->step_counter) return GATRES_E_BADARG;
    const UpdateArgs u = update_args(ts, nullptr, nullptr, false);
    return ts->autoclip ? autoclip_update(ts, u, stream) : gatres_adam_step_ex(u, stream);
  }
  return 0;
}
