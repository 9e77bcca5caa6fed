// smp_fit_policy.h -- the decision rule of the reference's two iterative training calls, as a pure host function: given the loss the
// loop has just evaluated, what happens.  No HIP, no handle, C++11: gf_smp_fit / gf_smp_model_fit (smp_fit.hip, smp_model.hip) drive
// the device with it, the CPU suite runs it on recorded loss sequences (tests/test_fit_policy.py, tests/cpp/fit_policy_sanitize.cpp).
//
// All 51 model headers of the reference share the two loops, down to the comparisons (GraphFlow/SMP_omega.h:827-922, GCN_1D.h:347-438):
//   kind 0, BatchLearn(nBatch, molecule, target, nIterations, learning_rate, epsilon):
//       first = second = loss of the batch; per iteration: one step, loss;  loss > second: restore, lr *= 0.5, leave when lr < 1e-6;
//       else second = loss, cache.  epsilon is not read.
//   kind 1, Learn(molecule, target, nIterations, learning_rate, epsilon):
//       best = loss of the sample; best < epsilon: return (best, best) at once; per iteration: one step, error;  error < epsilon: leave
//       (the step stays, best does not move);  error >= best: restore, lr = max(0.5 lr, 1e-6);  else best = error, cache.
//       Returns (first loss, best).
// A classifier's "loss" is its LogLoss value (<= 0); the reference applies the same comparisons to it, and so does this.
#ifndef GF_SMP_FIT_POLICY_H_INCLUDED
#define GF_SMP_FIT_POLICY_H_INCLUDED

namespace gf_fit {

enum Kind { kBatchLearn = 0, kLearn = 1 };
// what the loop does with the step it has just evaluated; the values are those of gf_smp_fit's decision log
enum Decision {
    kAccept = 1,       // keep the step: the loss becomes the one to beat, the parameters are cached
    kReject = 2,       // restore the cached parameters, halve the rate, go on
    kRejectLeave = 3,  // kind 0: restore, halve, and the rate is below 1e-6: leave the loop
    kLeave = 4         // kind 1: error < epsilon: leave the loop, the step stays
};

struct State {
    int kind;
    double learning_rate, epsilon;
    double first, second;   // the returned pair so far (kind 1: second = best_error)
    int iterations, accepted, rejected;
    bool left_early;        // a break, or kind 1's immediate return
};

inline double decay_lr() { return 0.5; }
inline double min_lr() { return 1e-6; }

// The loss before the first iteration.  false: the loop does not run at all (kind 1 with first_loss < epsilon).
inline bool begin(State *s, int kind, double learning_rate, double epsilon, double first_loss) {
    s->kind = kind;
    s->learning_rate = learning_rate;
    s->epsilon = epsilon;
    s->first = s->second = first_loss;
    s->iterations = s->accepted = s->rejected = 0;
    s->left_early = false;
    if (kind == kLearn && first_loss < epsilon) {
        s->left_early = true;
        return false;
    }
    return true;
}

// The loss after one more step at s->learning_rate.  The caller restores on kReject / kRejectLeave, caches on kAccept, and stops on
// kRejectLeave / kLeave.
inline Decision step(State *s, double loss) {
    ++s->iterations;
    if (s->kind == kBatchLearn) {
        if (loss > s->second) {
            ++s->rejected;
            s->learning_rate *= decay_lr();
            if (s->learning_rate < min_lr()) {
                s->left_early = true;
                return kRejectLeave;
            }
            return kReject;
        }
        s->second = loss;
        ++s->accepted;
        return kAccept;
    }
    if (loss < s->epsilon) {
        s->left_early = true;
        return kLeave;
    }
    if (loss >= s->second) {
        ++s->rejected;
        s->learning_rate *= decay_lr();
        s->learning_rate = s->learning_rate > min_lr() ? s->learning_rate : min_lr();   // max(learning_rate, min_lr)
        return kReject;
    }
    s->second = loss;
    ++s->accepted;
    return kAccept;
}

}  // namespace gf_fit
#endif
