// saturate_gate.cpp -- the host side of K1's saturation exit (dd_plan.h: plan_saturate_last_k, PlanKnobs; dd_kernels.h:
// universe_size) without a GPU, built with dd_plan.hip under -fsanitize=address,undefined by tests/test_saturate_gate.py.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dd_plan.h"

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                \
        }                                                              \
    } while (0)

static int gate(int log2m, int canon, int kmin, int kmax, const dd::PlanKnobs& kn, std::vector<size_t> sizes) {
    return dd::plan_saturate_last_k(log2m, canon, kmin, kmax, kn, sizes.data(), (int)sizes.size());
}

int main() {
    using dd::universe_size;
    // |U_k|: every k-mer, or one of each (k-mer, reverse complement) pair; only even k has palindromes
    for (int k = 1; k <= 14; ++k) {
        const size_t all = (size_t)1 << (2 * k), pal = (k & 1) ? 0 : (size_t)1 << k;
        CHECK(universe_size(k, false) == all);
        CHECK(universe_size(k, true) == (all - pal) / 2 + pal);
    }
    CHECK(universe_size(10, true) == 524800 && universe_size(11, true) == 2097152);

    const dd::PlanKnobs def;
    // the benchmark's call: 10 x 50 Mbp saturates k = 10 and 11, not 12 (8 |U_12| = 67 M)
    CHECK(gate(14, 1, 4, 40, def, std::vector<size_t>(10, 50625080)) == 11);
    CHECK(gate(16, 1, 4, 40, def, std::vector<size_t>(10, 50625080)) == 11);
    CHECK(gate(14, 0, 4, 40, def, std::vector<size_t>(10, 50625080)) == 11);   // 8 x 4^11 = 33.5 M
    CHECK(gate(14, 0, 4, 40, def, {30000000}) == 10);
    // the longest genome decides
    CHECK(gate(14, 1, 4, 40, def, {1000, 250000000, 0}) == 12);
    CHECK(gate(14, 1, 4, 40, def, {3000000000ull}) == 14);
    // exactly at the gate, and one byte under it
    CHECK(gate(14, 1, 4, 40, def, {8 * 524800}) == 10);
    CHECK(gate(14, 1, 4, 40, def, {8 * 524800 - 1}) == 0);
    // the call's k range
    CHECK(gate(14, 1, 4, 9, def, {3000000000ull}) == 0);
    CHECK(gate(14, 1, 4, 10, def, {3000000000ull}) == 10);
    CHECK(gate(14, 1, 12, 40, def, {3000000000ull}) == 14);
    CHECK(gate(14, 1, 12, 40, def, std::vector<size_t>(10, 50625080)) == 0);    // 10 and 11 would do, the call starts at 12
    CHECK(gate(14, 1, 15, 40, def, {3000000000ull}) == 0);
    // registers in LDS only; rows of 16 bytes at least
    CHECK(gate(17, 1, 4, 40, def, {3000000000ull}) == 0);
    CHECK(gate(20, 1, 4, 40, def, {3000000000ull}) == 0);
    CHECK(gate(3, 1, 4, 40, def, {3000000000ull}) == 0);
    CHECK(gate(4, 1, 4, 40, def, {3000000000ull}) == 14);
    CHECK(gate(14, 1, 4, 40, def, {}) == 0);
    // the knobs
    dd::PlanKnobs any, off, both;
    any.saturate_any_size = true;
    off.no_saturate = true;
    both.saturate_any_size = both.no_saturate = true;
    CHECK(gate(14, 1, 4, 40, any, {1000}) == 14);
    CHECK(gate(14, 1, 4, 12, any, {1000}) == 12);
    CHECK(gate(14, 1, 4, 9, any, {1000}) == 0);
    CHECK(gate(17, 1, 4, 40, any, {1000}) == 0);
    CHECK(gate(14, 1, 4, 40, off, {3000000000ull}) == 0);
    CHECK(gate(14, 1, 4, 40, both, {3000000000ull}) == 0);
    CHECK(!(def == any) && !(def == off) && !(any == both) && def == dd::PlanKnobs());
    // ... read from the environment, per call
    unsetenv("DD_SATURATE_ANY_SIZE");
    unsetenv("DD_NO_SATURATE");
    CHECK(dd::PlanKnobs::from_env() == def);
    setenv("DD_SATURATE_ANY_SIZE", "1", 1);
    CHECK(dd::PlanKnobs::from_env() == any);
    setenv("DD_NO_SATURATE", "1", 1);
    CHECK(dd::PlanKnobs::from_env() == both);
    unsetenv("DD_SATURATE_ANY_SIZE");
    CHECK(dd::PlanKnobs::from_env() == off);
    unsetenv("DD_NO_SATURATE");
    // the plan itself does not depend on either knob: same classes, same jobs in the same order
    const std::vector<size_t> sizes(3, 20000000);
    const auto a = dd::plan_sweep(14, 1, sizes.data(), 3, 4, 40, def), b = dd::plan_sweep(14, 1, sizes.data(), 3, 4, 40, both);
    CHECK(a.size() == b.size());
    for (size_t i = 0; i < a.size() && i < b.size(); ++i) {
        CHECK(a[i].kclass == b[i].kclass && a[i].jobs.size() == b[i].jobs.size() && a[i].plan.lds_bytes == b[i].plan.lds_bytes);
        for (size_t j = 0; j < a[i].jobs.size() && j < b[i].jobs.size(); ++j) {
            const dd::SweepJob &x = a[i].jobs[j], &y = b[i].jobs[j];
            CHECK(x.genome == y.genome && x.kfirst == y.kfirst && x.nk == y.nk && x.krow == y.krow && x.tile_begin == y.tile_begin &&
                  x.tile_end == y.tile_end);
        }
    }
    if (failures) return 1;
    printf("saturate_gate: ok\n");
    return 0;
}
