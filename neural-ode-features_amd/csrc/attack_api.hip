// C ABI of the basic-iterative attack's per-iteration arithmetic (include/node_hip.h: node_attack_step / node_attack_judge):
// argument checks and the launches of kernels_attack.hip.  Every refusal happens before the first HIP call.
#include "host_common.h"
#include "attack.h"

using namespace node;

namespace {
int check_attack(const node_attack* k) {
  if (!k) return fail(NODE_ERR_NULL, "attack description is NULL");
  if (k->n < 1 || k->c < 1 || k->h < 1 || k->w < 1) return fail(NODE_ERR_SHAPE, "attack shape n=%d c=%d h=%d w=%d", k->n, k->c, k->h, k->w);
  if ((int64_t)k->c * k->h * k->w >= ((int64_t)1 << 31)) return fail(NODE_ERR_UNSUPPORTED, "an image must stay under 2^31 elements");
  if (k->norm != NODE_ATTACK_LINF && k->norm != NODE_ATTACK_L2) return fail(NODE_ERR_ARG, "attack norm=%d: 0 (L-infinity) or 2 (L2)", k->norm);
  if (!(k->hi > k->lo)) return fail(NODE_ERR_ARG, "attack bounds lo=%g hi=%g: hi must exceed lo", k->lo, k->hi);
  if (!(k->epsilon >= 0.0) || !(k->stepsize >= 0.0)) return fail(NODE_ERR_ARG, "attack epsilon=%g stepsize=%g: both must be >= 0", k->epsilon, k->stepsize);
  if ((k->mean == nullptr) != (k->std == nullptr)) return fail(NODE_ERR_NULL, "attack mean and std: both or neither");
  return NODE_OK;
}
}  // namespace

extern "C" {

int node_attack_step(const node_attack* k, float* x, const float* x0, const float* g, const int32_t* active, float* x_norm,
                     void* stream) {
  int rc = check_attack(k);
  if (rc != NODE_OK) return rc;
  if (!x || !x0 || !g || !active || !x_norm) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  AttackStepArgs a;
  a.x = x; a.x0 = x0; a.g = g; a.mean = k->mean; a.std = k->std; a.active = active; a.xn = x_norm;
  a.c = k->c; a.hw = k->h * k->w; a.l2 = k->norm == NODE_ATTACK_L2;
  const double s = k->hi - k->lo;
  a.s = (float)s; a.stepsize = (float)k->stepsize; a.eps_s = (float)(k->epsilon * s); a.lo = (float)k->lo; a.hi = (float)k->hi;
  launch_attack_step(a, k->n, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of k_attack_step failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

int node_attack_judge(const node_attack* k, int classes, const float* logits, const int64_t* labels, const float* x, const float* x0,
                      int initial, int iteration, const node_attack_record* rec, void* stream) {
  int rc = check_attack(k);
  if (rc != NODE_OK) return rc;
  if (classes < 1) return fail(NODE_ERR_SHAPE, "attack classes=%d", classes);
  if (!logits || !labels || !x || !x0 || !rec) return fail(NODE_ERR_NULL, "a required pointer is NULL");
  if (!rec->active || !rec->original_class || !rec->adversarial_class || !rec->found_iteration || !rec->distance)
    return fail(NODE_ERR_NULL, "a field of the attack record is NULL");
  if (!k->return_early && !rec->best_x) return fail(NODE_ERR_NULL, "without return_early the record needs best_x");
  AttackJudgeArgs a;
  a.logits = logits; a.labels = labels; a.x = x; a.x0 = x0;
  a.active = rec->active; a.original_class = rec->original_class; a.adversarial_class = rec->adversarial_class;
  a.found_iteration = rec->found_iteration; a.distance = rec->distance; a.best_x = rec->best_x;
  a.classes = classes; a.d = k->c * k->h * k->w; a.l2 = k->norm == NODE_ATTACK_L2; a.initial = initial != 0; a.iteration = iteration;
  a.return_early = k->return_early != 0; a.s = (float)(k->hi - k->lo);
  launch_attack_judge(a, k->n, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NODE_ERR_HIP, "launch of k_attack_judge failed: %s", hipGetErrorString(e));
  return NODE_OK;
}

}  // extern "C"
