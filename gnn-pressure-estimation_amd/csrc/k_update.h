// The update launches that end a training step -- reduce_adam_kernel and param_grads_finish_kernel (k_fused_host.hip),
// adam_kernel (k_misc.hip), autoclip_adam_kernel (k_autoclip.hip) -- take ONE argument struct, and the hidden functions
// through which gatres_train_step (train_driver.hip) reaches them are declared here, once.
#pragma once
#include "gatres_common.h"

// What an update launch is given.  Zero-initialised it means plain Adam with nothing optional: a caller names what it uses.
struct UpdateArgs {
  // optimizer state, `count` floats each.  g is the gradient the update READS (adam_kernel, autoclip_adam_kernel); the fused
  // finish launches update with the slab sum they form themselves and write it through their own `grads` argument.
  float* p;
  const float* g;
  float* m;
  float* v;
  unsigned long long* step_counter;      // [0] = step, [1] = block ticket
  long long count;
  // hyper-parameters; hp: double[5] {lr, beta1, beta2, eps, weight_decay} in device memory (gatres_train_step_t.hparams)
  // that replaces the five by-value ones, or null
  double lr, b1, b2, eps, wd;
  const double* hp;
  float grad_scale;
  // the fused path's transposed conv weights, kept current by the update (transpose_conv_weights_kernel's layout), or null
  float* wt;
  int nb, nc;
  // the NEXT step's device mask, sampled by workgroups behind the update's (mask_next, or null: nothing is sampled).
  // mask_snap: {step count before this update, fault word}, stable during the launch -- the parameter-gradient launch of
  // this step left it in the status block (gatres_layout.h).
  const int* mask_node_ptr;
  int mask_graphs;
  double mask_rate;
  unsigned long long mask_seed;
  uint8_t* mask_next;
  const unsigned long long* mask_snap;
  // fault-marked steps (g[0] is NaN) are dropped and counted here (the data-parallel Adam phase of the fused path), or null
  unsigned* drop_count;
};

// The struct of a public entry point's positional arguments (include/gatres.h): the optimizer state and the hyper-parameters
static inline UpdateArgs update_args_of(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                        uint64_t* step_counter, int64_t count, double lr, double beta1, double beta2, double eps,
                                        double weight_decay, const double* hparams, float grad_scale) {
  UpdateArgs u{};
  u.p = params; u.g = grads; u.m = exp_avg; u.v = exp_avg_sq;
  u.step_counter = reinterpret_cast<unsigned long long*>(step_counter); u.count = count;
  u.lr = lr; u.b1 = beta1; u.b2 = beta2; u.eps = eps; u.wd = weight_decay; u.hp = hparams; u.grad_scale = grad_scale;
  return u;
}

// Adam with everything gatres_train_step may ask for (gatres_adam_step: the same launch with nothing optional)
extern "C" __attribute__((visibility("hidden"))) int gatres_adam_step_ex(const UpdateArgs& u, void* stream);

// The slab sum of the fused path and (do_adam) the update in the same launch; grads receives the sum.  use_snap: the
// parameter-gradient launch in front of this one (gatres_fused_param_grads_ex) left the step count / fault word snapshot:
// the update reads those instead of drawing tickets, and may sample the next mask.  u.count, u.wt / nb / nc and u.mask_snap
// are not the caller's to give: they follow from the layout and the scratch.
extern "C" __attribute__((visibility("hidden"))) int gatres_fused_finish_ex(
    const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads, const float* loss_part, float* loss,
    int32_t do_adam, const UpdateArgs& u, int32_t use_snap, void* stream);

// AutoClip: the norm launch, then the update launch (k_autoclip.hip).  The norm launch is the stand-alone one over a complete
// gradient (u.g; a NaN in g[0] drops the step where u.drop_count is set) or, on the fused path, the slab sum itself
// (gatres_fused_finish_ex without Adam; uses u.step_counter and u.grad_scale).  *num_partials = partials it leaves.
extern "C" __attribute__((visibility("hidden"))) int gatres_autoclip_norm_ex(const UpdateArgs& u, const gatres_autoclip_t* ac,
                                                                             int32_t* num_partials, void* stream);
extern "C" __attribute__((visibility("hidden"))) int gatres_fused_finish_norm_ex(
    const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads, const float* loss_part, float* loss,
    const UpdateArgs& u, const gatres_autoclip_t* ac, int32_t* num_partials, void* stream);
extern "C" __attribute__((visibility("hidden"))) int gatres_autoclip_update_ex(const UpdateArgs& u, const gatres_autoclip_t* ac,
                                                                               int32_t num_partials, void* stream);
