"""Completeness of the capture / side-stream conformance table (tests/_capture_cases.py): every entry point of include/dprhot.h that
takes a `void* stream` is exercised by a row of the table, or is one of the six RCCL collectives, which are excluded by name with the
reason recorded next to the list.  Host code only: the header is parsed, nothing is launched."""
import os
import re
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _capture_cases as CC  # noqa: E402

COLLECTIVES = {"dprhot_allgather_ctx", "dprhot_reducescatter_dc", "dprhot_reducescatter_rows", "dprhot_allreduce_sum",
               "dprhot_allgather_allpairs", "dprhot_reducescatter_allpairs"}


def stream_entry_points():
    """Every prototype dprhot_<name>(...) of the header whose parameter list holds `void* stream`, comments stripped first."""
    with open(os.path.join(ROOT, "include", "dprhot.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = re.findall(r"\b(dprhot_\w+)\s*\(([^()]*)\)\s*;", text)
    return {name for name, params in protos if re.search(r"\bvoid\s*\*\s*stream\b", params)}


def test_the_header_has_the_entry_points_this_table_was_written_for():
    assert len(stream_entry_points()) == 69


def test_every_stream_taking_entry_point_is_covered_or_excluded_by_name():
    declared = stream_entry_points()
    assert set(CC.EXCLUDED) == COLLECTIVES and all("communicator" in why for why in CC.EXCLUDED.values())
    covered = CC.covered()
    assert not covered & set(CC.EXCLUDED), "an excluded entry point has a row"
    assert covered | set(CC.EXCLUDED) == declared, (sorted(declared - covered - set(CC.EXCLUDED)), sorted(covered - declared))
    assert len(covered) == 63 and len(CC.EXCLUDED) == 6


def test_rows_are_named_once_and_declare_symbols():
    names = [c.name for c in CC.CASES]
    assert len(names) == len(set(names)) and all(c.symbols for c in CC.CASES)
