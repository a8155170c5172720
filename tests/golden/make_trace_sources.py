#!/usr/bin/env python3
"""Regenerates tests/golden/trace_sources.json: the digests of what the three density tracers (bayes_kit_amd.trace,
trace_lanes, trace_chain) generate and refuse on the corpus of tests/test_trace_cpu.py, with the torch version they hold for.

    python tests/golden/make_trace_sources.py          # no GPU; two runs give the same file

Only for a DELIBERATE change of the generated text or of a message: the fixture is what says a refactor changed neither.
"""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
for p in (ROOT, os.path.join(ROOT, "bayes-kit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from tests import test_trace_cpu as corpus  # noqa: E402

if __name__ == "__main__":
    with open(corpus.TRACE_PINS, "w") as f:
        json.dump({"torch": torch.__version__, "digests": corpus.trace_pins()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", corpus.TRACE_PINS)
