"""The library's environment switches are read in one place, hnsw_rs_amd/csrc/switches.h: nothing else under csrc/
calls getenv, every HNSW_MI355X_* name that the tests, bench.py and the scripts use is declared there, and the two
retired switches are not.  File reading only: no GPU, no compiler."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hnsw_rs_amd", "csrc")
NAME = re.compile(r"HNSW_MI355X_[A-Z0-9_]+")
# not the library's: the path of the shared library (hnsw_rs_amd/_lib.py reads it) and a switch of a variant that was
# never kept, named in a script's docstring
NOT_THE_LIBRARYS = {"HNSW_MI355X_LIB", "HNSW_MI355X_HELPERS"}
RETIRED = {"HNSW_MI355X_WAVES", "HNSW_MI355X_LIST"}


def read(path):
    return open(path, errors="replace").read()


def declared():
    return set(NAME.findall(read(os.path.join(CSRC, "switches.h"))))


def test_getenv_is_called_in_switches_h_alone():
    others = [p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.basename(p) != "switches.h" and
              os.path.splitext(p)[1] in (".cpp", ".hip", ".h", ".inc")]  # (the sources: objects of a build lie beside them)
    assert len(others) > 30, others
    assert [os.path.basename(p) for p in others if "getenv" in read(p)] == []
    assert "getenv" in read(os.path.join(CSRC, "switches.h"))


def test_every_switch_in_use_is_declared():
    users = ([os.path.join(ROOT, "bench.py")] + glob.glob(os.path.join(ROOT, "scripts", "*.py")) +
             glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True))
    used = {}
    for p in users:
        if os.path.abspath(p) == os.path.abspath(__file__):
            continue
        for name in NAME.findall(read(p)):
            used.setdefault(name, os.path.relpath(p, ROOT))
    assert "HNSW_MI355X_LEAN" in used and "HNSW_MI355X_INSERT_TABLE_ADJUST" in used, used
    have = declared()
    assert {n: p for n, p in used.items() if n not in have | NOT_THE_LIBRARYS} == {}


def test_the_retired_switches_are_gone():
    assert declared() & RETIRED == set()
