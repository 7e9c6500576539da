// rt_query_form.h -- which of its eight forms a triangle query kernel runs in for a scene, decided on the host in one place for
// every family (rt_query.hip, rt_shade.hip, rt_sample.hip, rt_gbuffer.hip, rt_ao.hip: the kernels templated on
// <STK, PACKED, PAIRS, P16, INST>, as trace_tlas is).  Every form computes the same bits, so no result can tell which one ran:
// tests/c/query_form_test.cpp prints the choice for the whole input space and tests/test_query_form_cpu.py holds it against the
// rule written out.  Host-only, no HIP.
//
// The rule.  INST: the instance data travels with the call (query_prepare's `inst`) and the kernel stages it from its arguments.
//   pairs: the relinked pair records -- only with every instance staged (the root's meta rides in its record), as in the frame
//     kernels: inst, records present and current, 16-bit node indices, a packed walk, at most `wide_blas` instances.
//       pairs and p16_ok: <uint16_t, packed, pairs, p16, inst>;  pairs alone: <uint16_t, packed, pairs, -, inst>
//   otherwise the node walk, with INST = inst:
//       n_nodes <= 65536 and packed_ok: <uint16_t, packed, -, -, INST>;  n_nodes <= 65536: <uint16_t, -, -, -, INST>;
//       any larger tree: <uint32_t, -, -, -, INST>
#pragma once
#include <cstdint>

// one form: the template arguments of a triangle query kernel
template <typename STK_, bool PACKED_, bool PAIRS_, bool P16_, bool INST_>
struct RtQueryForm {
    typedef STK_ STK;
    static constexpr bool PACKED = PACKED_, PAIRS = PAIRS_, P16 = P16_, INST = INST_;
};

// calls f(RtQueryForm<...>()) once, with the form of the scene; wide_blas: rt_tri_device.h kWideBlas
template <typename F>
inline void rt_query_form(bool inst, bool have_pairs, uint32_t n_nodes, bool packed_ok, bool p16_ok, uint32_t n_blas, uint32_t wide_blas,
                          F&& f) {
    const bool pairs = inst && have_pairs && n_nodes <= 65536u && packed_ok && n_blas <= wide_blas;
    if (pairs && p16_ok) f(RtQueryForm<uint16_t, true, true, true, true>());
    else if (pairs)      f(RtQueryForm<uint16_t, true, true, false, true>());
    else if (inst) {
        if (n_nodes <= 65536u && packed_ok) f(RtQueryForm<uint16_t, true, false, false, true>());
        else if (n_nodes <= 65536u)         f(RtQueryForm<uint16_t, false, false, false, true>());
        else                                f(RtQueryForm<uint32_t, false, false, false, true>());
    } else {
        if (n_nodes <= 65536u && packed_ok) f(RtQueryForm<uint16_t, true, false, false, false>());
        else if (n_nodes <= 65536u)         f(RtQueryForm<uint16_t, false, false, false, false>());
        else                                f(RtQueryForm<uint32_t, false, false, false, false>());
    }
}
