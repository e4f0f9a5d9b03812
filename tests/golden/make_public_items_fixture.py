"""Read the public surface of the reference's `hnsw` crate off its source tree into a data fixture.

    python tests/golden/make_public_items_fixture.py <reference checkout>
Writes tests/golden/reference_public_items.json: the names of every `pub fn` of hnsw/src/template.rs and
hnsw/src/helpers/args.rs, and every `use hnsw::...` path of eval_glove/src/main.rs and
hnsw/benches/hnsw_benchmarks.rs.  tests/test_shim_surface.py checks its own lists against these names, so
the suite does not need the reference tree to run.  These are DATA (names), not code.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_public_items.json")
PUB_FN_FILES = {"template_pub_fns": "hnsw/src/template.rs", "args_pub_fns": "hnsw/src/helpers/args.rs"}
CALLER_FILES = ("eval_glove/src/main.rs", "hnsw/benches/hnsw_benchmarks.rs")


def pub_fns(src):
    return sorted(set(re.findall(r"pub fn\s+([A-Za-z_0-9]+)", src)))


def caller_imports(paths):
    imports = set()
    for path in paths:
        for line in open(path):
            m = re.match(r"\s*use (hnsw::[A-Za-z_:0-9]+);", line)
            if m:
                imports.add(m.group(1))
    return sorted(imports)


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "hnsw", "src")):
        sys.exit("usage: make_public_items_fixture.py <checkout of the reference hnsw_rs tree>")
    ref = sys.argv[1]
    doc = {k: pub_fns(open(os.path.join(ref, f)).read()) for k, f in PUB_FN_FILES.items()}
    doc["caller_imports"] = caller_imports([os.path.join(ref, f) for f in CALLER_FILES])
    doc["read_from"] = dict(PUB_FN_FILES, caller_imports=list(CALLER_FILES))
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %s" % (OUT, {k: len(v) for k, v in doc.items() if k != "read_from"}))
