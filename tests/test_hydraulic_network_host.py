"""The valves, emitters and pressure-driven-demand launches are stated once (csrc/k_hydraulic_network.hip around the Newton loop of
csrc/k_hydraulics_dev.h): the three files that restated them are gone, the loop stays in the header, every helper the hydraulic
sources share has one definition, and the six entry points keep their places in gatres.h, in the library and in ``_native``.
Reads csrc/ and include/gatres.h.  No GPU."""
import os
import re

import pytest

import gnn_pressure_estimation_amd as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = G._build.CSRC
GONE = ("k_hydraulic_valves.hip", "k_hydraulic_emitters.hip", "k_hydraulic_pdd.hip")
ONCE = ("hy_set_speed(double*", "hy_link_code(const HyLds&", "hy_link_state(int", "hy_check_valve_links(const",
        "hy_check_emitters(const", "hy_valve_start(const", "hy_emitter_start(const", "bytes_overlap(const void*",
        "any_overlap(const void*", "hy_counts_ok(int64_t")
ENTRY_POINTS = {"gatres_hydraulic_solve_valves": 43, "gatres_hydraulic_series_valves": 60, "gatres_hydraulic_solve_emitters": 49,
                "gatres_hydraulic_series_emitters": 68, "gatres_hydraulic_solve_pdd": 54, "gatres_hydraulic_series_pdd": 73}


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}


def test_the_three_restatements_are_gone_and_the_one_file_is_built():
    files = os.listdir(CSRC)
    for name in GONE:
        assert name not in files and name not in G._build.SOURCES
    assert "k_hydraulic_network.hip" in files and G._build.SOURCES.count("k_hydraulic_network.hip") == 1
    assert all(os.path.exists(os.path.join(CSRC, s)) for s in G._build.SOURCES)


def test_the_newton_loop_stays_in_the_header():
    src = _sources()
    assert not [f for f, text in src.items() if f.endswith(".hip") and "for (int it = 1;" in text]
    assert src["k_hydraulics_dev.h"].count("for (int it = 1;") == 2      # hy_newton and hy_newton_valves


@pytest.mark.parametrize("signature", ONCE)
def test_a_shared_helper_is_defined_exactly_once(signature):
    where = {f: text.count(signature) for f, text in _sources().items() if signature in text}
    assert sum(where.values()) == 1, where


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_an_entry_point_is_declared_exported_and_bound_with_its_arguments(name):
    header = open(os.path.join(ROOT, "include", "gatres.h")).read()
    m = re.search(r"\bint " + name + r"\(([^;]*?)\);", header, re.S)
    assert m and m.group(1).count(",") + 1 == ENTRY_POINTS[name]
    assert len(G._native.SIGNATURES[name][1]) == ENTRY_POINTS[name]
    text = _sources()["k_hydraulic_network.hip"]
    assert len(re.findall(r'extern "C" int ' + name + r"\(", text)) == 1
    fn = getattr(G._native.load(), name)                    # exported by the library, bound with the signature
    assert len(fn.argtypes) == ENTRY_POINTS[name]
    assert "#define GATRES_ABI_VERSION 9" in header and G._native.ABI_VERSION == 9
