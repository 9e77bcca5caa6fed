// The decision rule of gf_smp_fit (graphflow_amd/csrc/smp_fit_policy.h) as a stand-alone program: no HIP, no handle.
//   fit_policy_sanitize                 built-in sequences: every branch of both kinds, NaN and infinite losses, no iterations; prints PASSED
//   fit_policy_sanitize <file>          one loop per line of <file>:  kind nIterations learning_rate epsilon first_loss loss...
//                                       (doubles as hexadecimal floats); per loop one line out:
//                                       first second final_rate iterations accepted rejected left_early decisions...
// tests/test_fit_policy.py feeds it the loss sequences the reference's classes produced (tests/golden/smp_iterative.npz), and runs it
// under AddressSanitizer + UBSan.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "smp_fit_policy.h"

// the loop of gf::fit_run, the device taken out: the losses come from the caller, in order, one per iteration run
static gf_fit::State run(int kind, int nIterations, double lr, double epsilon, double first, const std::vector<double> &losses,
                         std::vector<int> *decisions) {
    gf_fit::State s;
    decisions->clear();
    if (!gf_fit::begin(&s, kind, lr, epsilon, first)) return s;
    for (int iter = 0; iter < nIterations && iter < (int)losses.size(); ++iter) {
        const gf_fit::Decision d = gf_fit::step(&s, losses[iter]);
        decisions->push_back((int)d);
        if (d == gf_fit::kRejectLeave || d == gf_fit::kLeave) break;
    }
    return s;
}

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static void built_in() {
    std::vector<int> d;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // kind 0: keep, restore, keep on an equal loss (`>` is strict), epsilon is not read
    gf_fit::State s = run(0, 4, 0.5, 1e300, 10.0, {8.0, 9.0, 8.0, 7.0}, &d);
    CHECK((d == std::vector<int>{1, 2, 1, 1}) && s.first == 10.0 && s.second == 7.0 && s.learning_rate == 0.25 && s.accepted == 3 && s.rejected == 1 && !s.left_early);
    // kind 0: 2e-6 -> 1e-6 is NOT below the floor, -> 5e-7 is
    s = run(0, 10, 2e-6, 0.0, 1.0, {2.0, 2.0, 2.0}, &d);
    CHECK((d == std::vector<int>{2, 3}) && s.left_early && s.iterations == 2 && s.second == 1.0 && s.learning_rate == 5e-7);
    // kind 0: a NaN loss compares false with `>`: the reference keeps it, and so does this
    s = run(0, 2, 0.1, 0.0, 1.0, {nan, 0.5}, &d);
    CHECK((d == std::vector<int>{1, 1}) && s.second == 0.5);
    s = run(0, 1, 0.1, 0.0, 1.0, {inf}, &d);
    CHECK((d == std::vector<int>{2}) && s.second == 1.0 && s.learning_rate == 0.05);
    // kind 1: the immediate return, and `<` is strict there
    s = run(1, 5, 0.1, 2.0, 1.0, {0.5}, &d);
    CHECK(d.empty() && s.left_early && s.iterations == 0 && s.first == 1.0 && s.second == 1.0);
    s = run(1, 1, 0.1, 1.0, 1.0, {3.0}, &d);
    CHECK((d == std::vector<int>{2}) && !s.left_early);
    // kind 1: an equal error is restored (`>=`), the rate stops at 1e-6 and the loop goes on, error < epsilon leaves with best unmoved
    s = run(1, 6, 3e-6, 0.25, 4.0, {4.0, 5.0, 3.0, 3.0, 0.2, 0.1}, &d);
    CHECK((d == std::vector<int>{2, 2, 1, 2, 4}) && s.left_early && s.second == 3.0 && s.learning_rate == 1e-6 && s.iterations == 5 && s.accepted == 1 && s.rejected == 3);
    // kind 1: LogLoss values (<= 0) under the same comparisons; NaN is neither below epsilon nor `>=` best: kept
    s = run(1, 3, 0.5, -10.0, -1.0, {-0.5, -2.0, nan}, &d);
    CHECK((d == std::vector<int>{2, 1, 1}) && s.learning_rate == 0.25 && std::isnan(s.second));
    // no iterations
    s = run(0, 0, 0.5, 0.0, 3.0, {}, &d);
    CHECK(d.empty() && s.first == 3.0 && s.second == 3.0 && !s.left_early && s.learning_rate == 0.5);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        built_in();
        std::printf(failures ? "%d checks FAILED\n" : "PASSED\n", failures);
        return failures ? 1 : 0;
    }
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    std::string text;
    char buf[4096];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    std::fclose(f);
    std::istringstream lines(text);
    std::string line;
    while (std::getline(lines, line)) {
        std::istringstream in(line);
        std::string tok;
        std::vector<double> v;
        while (in >> tok) v.push_back(std::strtod(tok.c_str(), NULL));
        if (v.empty()) continue;
        if (v.size() < 5) return 3;
        std::vector<int> d;
        const std::vector<double> losses(v.begin() + 5, v.end());
        const gf_fit::State s = run((int)v[0], (int)v[1], v[2], v[3], v[4], losses, &d);
        std::printf("%a %a %a %d %d %d %d", s.first, s.second, s.learning_rate, s.iterations, s.accepted, s.rejected, s.left_early ? 1 : 0);
        for (size_t i = 0; i < d.size(); ++i) std::printf(" %d", d[i]);
        std::printf("\n");
    }
    return 0;
}
