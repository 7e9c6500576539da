"""The form ladder of the triangle query kernels without a GPU: which of the eight <STK, PACKED, PAIRS, P16, INST> forms a scene
gets is decided by the host-only header compute_raytracer_amd/csrc/rt_query_form.h, once for all seven families.  Every form
computes the same bits, so no result shows which one ran -- a wrong choice would only be slower.  tests/c/query_form_test.cpp
prints the choice for every combination of the inputs at their thresholds; here it is held against the rule written out."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_BLAS = 16


def expected(inst, pairs, n_nodes, packed_ok, p16_ok, n_blas):
    """(sizeof STK, PACKED, PAIRS, P16, INST)"""
    use_pairs = inst and pairs and n_nodes <= 65536 and packed_ok and n_blas <= WIDE_BLAS
    if use_pairs and p16_ok:
        return (2, 1, 1, 1, 1)
    if use_pairs:
        return (2, 1, 1, 0, 1)
    if n_nodes <= 65536 and packed_ok:
        return (2, 1, 0, 0, inst)
    if n_nodes <= 65536:
        return (2, 0, 0, 0, inst)
    return (4, 0, 0, 0, inst)


def test_every_input_gets_the_form_the_rule_names(tmp_path):
    exe = str(tmp_path / "query_form_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "query_form_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        key, form = line.split(":")
        got[tuple(int(x) for x in key.split())] = tuple(int(x) for x in form.split())
    cases = list(itertools.product((0, 1), (0, 1), (1, 65536, 65537), (0, 1), (0, 1), (1, 16, 17)))
    assert len(cases) == 144 and len(r.stdout.splitlines()) == 144 and sorted(got) == sorted(cases)
    for case in cases:
        assert got[case] == expected(*case), (case, got[case], expected(*case))
    assert len(set(got.values())) == 8              # every form is reached
