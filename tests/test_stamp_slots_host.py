"""The stamps build's slot table (hnsw_rs_amd/csrc/stamp_slots.inc) and its readers (no GPU, no compiler).
DESIGN.md section 10 and the files under profiles/ cite slots by number, so the numbers the slots had before they
had names are pinned here; the diagnostic scripts index the side buffer by name, so every name they use must be in
the table; and the kernels name events on single lines, so no stamp #ifdef may come back into a kernel file."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hnsw_rs_amd", "csrc")


def _table():
    spec = importlib.util.spec_from_file_location("stamp_slots", os.path.join(ROOT, "scripts", "stamp_slots.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _table()


def test_the_table_parses_and_is_consistent():
    assert T.STRIDE == 64
    assert set(T.LISTS) == {"LEAN", "MERGE", "Q8", "FAT", "GENERIC", "PAIR"}
    for kernel, rows in T.LISTS.items():
        names = [r[0] for r in rows]
        numbers = [r[1] for r in rows]
        assert len(set(names)) == len(names), kernel
        assert len(set(numbers)) == len(numbers), kernel
        assert all(0 <= n < T.STRIDE for n in numbers), kernel
        assert all(r[2].strip() for r in rows), kernel
        assert T.slots(kernel) == dict(zip(names, numbers))
        assert T.descriptions(kernel) == {r[1]: r[2] for r in rows}
    # every X(...) line of the file was read: none is lost to a form the regular expression does not take
    text = open(T.TABLE).read()
    assert len(re.findall(r"^\s*X\(", text, re.M)) == sum(len(r) for r in T.LISTS.values())
    # a merge's five values from either base stay inside the buffer and off every other LEAN slot
    lean, merge = T.slots("LEAN"), T.slots("MERGE")
    assert sorted(merge.values()) == [0, 1, 2, 3, 4]
    split = {lean[b] + o for b in ("MERGE_C", "MERGE_P") for o in merge.values()}
    assert len(split) == 10 and max(split) < T.STRIDE
    assert split & set(lean.values()) == {lean["MERGE_C"], lean["MERGE_P"]}


def test_the_historical_numbers_are_kept():
    lean = T.slots("LEAN")
    pinned = {"PICK": 0, "FILTER": 1, "ROW_WAIT": 2, "CHAIN": 3, "TOTAL": 4, "COMMIT_P": 5, "PASSES": 6, "FRONT": 7,
              "MERGE_C_ALL": 8, "IS_P_NEXT": 9, "MERGE_P_ALL": 10, "SLOW_ROUNDS": 11, "MERGES_0": 12, "MERGES_1_2": 13,
              "MERGES_3_UP": 14, "P_COMMITS": 15, "MISS_1": 16, "MISS_2": 17, "MISS_3_UP": 18, "MISS_PREDICTED": 19,
              "MISS_OLD_P": 20, "PICK_AHEAD": 21, "PASSES_AHEAD": 22, "FILTER_KEPT": 23, "PASSES_KEPT": 24, "ENTRY": 25,
              "MERGE_C": 26, "MERGE_P": 31, "SMALL_C": 36, "SMALL_C_KEYS": 37, "SMALL_P": 38, "SMALL_P_KEYS": 39,
              "F_STAGING": 40, "F_CLEAR": 41, "F_ROW_WAIT": 42, "F_FILTER": 43, "F_ROWS_LEFT": 44, "F_CHAIN": 45,
              "F_TABLE": 47, "F_EXPANSIONS": 48,
              # the frontier's three: where the HX_STAMPS_FRONT build had them
              "FRONTIER": 50, "FRONTIER_RUNS": 51, "FRONTIER_RERUNS": 52}
    assert lean == pinned
    assert T.slots("MERGE") == {"LOOP": 0, "LDS": 1, "SHIFT": 2, "SURVIVORS": 3, "BIG": 4}
    assert T.slots("Q8") == {"PICK": 0, "FILTER": 1, "CHAIN": 3, "TOTAL": 4, "PASSES": 6, "FRONT": 7, "MERGE": 8}
    assert T.slots("FAT") == {"PICK": 0, "FILTER_HIT": 1, "CHAIN": 2, "MERGE": 3, "TOTAL": 4, "FILTER_MISS": 5, "HITS": 6}
    assert T.slots("GENERIC") == {"PICK": 0, "FILTER": 1, "ROW_WAIT": 2, "CHAIN": 3, "TOTAL": 4, "MERGE_C": 5,
                                  "COMMIT_P": 6, "PASSES": 7}
    assert T.slots("PAIR") == {"W_GATHER": 0, "W_WAIT_F": 1, "W_CLAIMS_P": 2, "W_SEND": 3, "W_CHECK_NEXT": 4, "W_LAYER0": 5,
                               "W_PASSES": 6, "W_TOTAL": 7, "K_WAIT_KEYS": 8, "K_MERGES": 9, "K_F": 10, "W_CHECK": 11}


# script -> the lists it reads
SCRIPTS = {"stamps_lean.py": ("LEAN", "MERGE"), "stamps_q8.py": ("Q8",), "stamps.py": ("FAT",), "stamps_f32.py": ("GENERIC",),
           "latency_floor.py": ("LEAN",), os.path.join("experiments", "pair_stamps.py"): ("PAIR",)}
# upper-case string literals of the scripts that are no slot names: environment variables and the lists' own tags
NOT_SLOTS = {"HX_DBG_PTR", "HX_STAMPS_FRONT", "LEAN", "MERGE", "Q8", "FAT", "GENERIC", "PAIR"}


def test_every_reader_of_the_side_buffer_is_held_to_the_table():
    # a script that hands the library a side buffer (HX_DBG_PTR) must size it by the table: a kernel writes at the
    # table's stride whatever the script believes, so a reader that is not listed above is a write out of bounds
    readers = set()
    for d, _, files in os.walk(os.path.join(ROOT, "scripts")):
        for f in files:
            if f.endswith(".py") and "HX_DBG_PTR" in open(os.path.join(d, f)).read():
                readers.add(os.path.relpath(os.path.join(d, f), os.path.join(ROOT, "scripts")))
    assert readers == set(SCRIPTS)


def test_the_scripts_use_names_the_table_has_and_no_numbers():
    for script, lists in SCRIPTS.items():
        text = open(os.path.join(ROOT, "scripts", script)).read()
        assert "from stamp_slots import" in text, script
        assert re.search(r"torch\.zeros\(\(nq, STRIDE\)", text), script
        known = set().union(*(T.slots(k) for k in lists))
        used = set(re.findall(r"""['"]([A-Z][A-Z0-9_]*)['"]""", text)) - NOT_SLOTS
        assert len(used) >= 5, (script, used)
        assert used <= known, (script, sorted(used - known))
        # the side buffer is indexed by name: no subscript of D holds a digit
        assert not re.findall(r"\bD\[[^\]]*\d[^\]]*\]", text), script


def test_no_stamp_ifdef_in_a_kernel_file():
    for f in ("search_lean.hip", "search_kernels.hip", "pair_kernel.inc"):
        text = open(os.path.join(CSRC, f)).read()
        assert not re.search(r"#\s*ifn?def\s+HX_STAMPS|#\s*(el)?if\b.*defined\s*\(?\s*HX_STAMPS", text), f
        assert not re.search(r"\bdbg_acc\b|\bt_begin\b|\bpp\[", text), f
