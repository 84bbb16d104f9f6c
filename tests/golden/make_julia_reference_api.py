#!/usr/bin/env python3
"""Generate tests/golden/julia_reference_api.json: what tests/test_julia_ext_vs_reference.py needs to know about the
reference's Julia sources, so that the test runs from this repository alone.

The reference's src/*.jl is read as text by the test module's own regex parser; the file holds DATA only -- struct field
names, the (min, max) positional arities of every method, the other top-level names (abstract types, consts), the
third-party names the parent brings into its namespace, the argument counts of the parent's calls of its bare stubs, and
the sequence of collectives in the parent's VectorPlan constructor.  No source text is stored.

Run:  python tests/golden/make_julia_reference_api.py REFERENCE_TREE   (the directory that holds the reference's src/)
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import test_julia_ext_vs_reference as t  # noqa: E402


def extract(ref_dir):
    text = t.reference_text(ref_dir)
    structs = t.reference_structs(text)
    functions = t.reference_functions(text)
    m = re.search(t.REF_VECTORPLAN_HEADER, text, flags=re.M)
    assert m, "the reference's VectorPlan constructor was not found"
    return {
        "structs": structs,
        "functions": {n: [list(a) for a in ar] for n, ar in sorted(functions.items())},
        "names": sorted(t.reference_names(text)),
        "third_party_names": sorted(t._third_party_names(text)),
        "stub_call_arities": t.stub_call_arities(text),
        "vectorplan_constructor_collectives": [list(c) for c in t._collectives(t._function_body(text, t.REF_VECTORPLAN_HEADER))],
    }


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "src")):
        raise SystemExit(__doc__)
    with open(os.path.join(HERE, "julia_reference_api.json"), "w") as f:
        json.dump(extract(sys.argv[1]), f, indent=1, sort_keys=True)
        f.write("\n")
