// The basic-iterative attack's per-iteration arithmetic (kernels_attack.hip; checks: attack_api.hip): internal declarations.
#pragma once
#include "node_internal.h"

namespace node {

constexpr int ATTACK_THREADS = 256;

struct AttackStepArgs {
  float* x;              // [n][c][hw] pixel space, updated in place
  const float* x0;       // the originals
  const float* g;        // gradient of the loss with respect to the normalised model input
  const float* mean;     // nullable [c]
  const float* std;      // nullable [c]
  const int32_t* active; // [n]
  float* xn;             // [n][c][hw]: the next model input (x - mean) / std
  int c, hw, l2;
  float s, stepsize, eps_s, lo, hi;     // s = hi - lo; eps_s = epsilon * s
};
void launch_attack_step(const AttackStepArgs& a, int n, hipStream_t s);

struct AttackJudgeArgs {
  const float* logits;   // [n][classes]
  const int64_t* labels; // [n]
  const float* x;        // [n][d]
  const float* x0;
  int32_t* active;
  int32_t* original_class;
  int32_t* adversarial_class;
  int32_t* found_iteration;
  float* distance;
  float* best_x;         // nullable with return_early: [n][d], the image behind `distance`
  int classes, d, l2, initial, iteration, return_early;
  float s;
};
void launch_attack_judge(const AttackJudgeArgs& a, int n, hipStream_t s);

}  // namespace node
