// The form a triangle query kernel runs in (compute_raytracer_amd/csrc/rt_query_form.h), printed for the whole input space: one line
// "inst pairs n_nodes packed_ok p16_ok n_blas : sizeof(STK) PACKED PAIRS P16 INST" per case.  Built and run by
// tests/test_query_form_cpu.py, which holds the table against the rule written out.
#include <cstdio>

#include "../../compute_raytracer_amd/csrc/rt_query_form.h"

int main() {
    const uint32_t kWideBlas = 16u;            // = rt_tri_device.h kWideBlas
    const uint32_t nodes[3] = {1u, 65536u, 65537u}, blas[3] = {1u, 16u, 17u};
    for (int inst = 0; inst < 2; ++inst)
        for (int pairs = 0; pairs < 2; ++pairs)
            for (uint32_t n_nodes : nodes)
                for (int packed_ok = 0; packed_ok < 2; ++packed_ok)
                    for (int p16_ok = 0; p16_ok < 2; ++p16_ok)
                        for (uint32_t n_blas : blas) {
                            int calls = 0;
                            rt_query_form(inst != 0, pairs != 0, n_nodes, packed_ok != 0, p16_ok != 0, n_blas, kWideBlas, [&](auto f) {
                                typedef decltype(f) F;
                                ++calls;
                                std::printf("%d %d %u %d %d %u : %zu %d %d %d %d\n", inst, pairs, n_nodes, packed_ok, p16_ok, n_blas,
                                            sizeof(typename F::STK), (int)F::PACKED, (int)F::PAIRS, (int)F::P16, (int)F::INST);
                            });
                            if (calls != 1) { std::printf("FAILED: %d calls\n", calls); return 1; }
                        }
    return 0;
}
