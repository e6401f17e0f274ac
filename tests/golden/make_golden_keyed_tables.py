"""Characterisation fixture of the host layer of the keyed evaluation calls (scanpaths_amd/utils/evaluation.py from likelihood_evaluation
down, the sum tables, and the batch loops of scanpaths_amd/inference.py), CPU only:

    python tests/golden/make_golden_keyed_tables.py

The device entry points are replaced by the deterministic stand-ins of tests/keyed_tables_cases.py, whose values are dyadic rationals:
what is recorded is what the host code makes of them -- pooled means, per-key tables, merged tables, refusal messages and, per batch
loop, how the model was called.  The log-based saccade and turn entries (keyed_tables_cases.DERIVED) are not stored: the test recomputes them
in-process.  Record it with the code whose behaviour is to be kept, BEFORE changing that code; the test then holds the changed code to it.
Writes tests/golden/keyed_tables.npz."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import keyed_tables_cases as C  # noqa: E402
from helpers import save_npz  # noqa: E402

if __name__ == "__main__":
    C.install(setattr)
    flat = {k: v for k, v in C.flatten(C.collect(setattr)).items() if not C.is_derived(k)}
    save_npz(os.path.join(HERE, "keyed_tables.npz"), C.pack(flat))
    print(f"{len(flat)} entries -> tests/golden/keyed_tables.npz, {os.path.getsize(os.path.join(HERE, 'keyed_tables.npz'))} bytes")
