"""Record what the REFERENCE build (oracle/_ref, built by oracle/Makefile from the reference's sources) returns in the tests that compare
with it, into tests/golden/ref_recordings.npz.  Where oracle/_ref is not built those tests read the recording instead (tests/helpers.py:
ref_arrays, RefScalars).  Runs where the reference's sources are; the tests are run against the live build with GBRL_RECORD_REF set, every
process writes what the reference returned to its own file, and the files are merged here.

    python tests/golden/make_ref_recordings.py
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402

TESTS = ["tests/test_oracle.py::test_restatement_matches_reference_build_live",
         "tests/test_oracle.py::test_restatement_agrees_with_the_reference_build_beyond_the_fixtures",
         "tests/test_oracle.py::test_replay_sequence_is_the_reference_functions_bit_for_bit",
         "tests/test_oracle.py::test_categorical_scores_follow_the_same_sequence",
         "tests/test_oracle.py::test_restatement_takes_the_references_side_of_a_mirror_tie",
         "tests/test_host.py::test_model_file_of_a_fresh_model_is_the_file_the_reference_writes",
         "tests/test_host.py::test_model_file_written_here_loads_in_the_reference",
         "tests/test_host.py::test_python_signatures_match_the_reference_class"]


def main():
    assert oracle.load_ref() is not None and oracle.ref_score_probe() is not None, "oracle/_ref is not built here"
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, GBRL_RECORD_REF=d)
        subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + TESTS, cwd=ROOT, env=env, check=True)
        merged = {}
        for f in sorted(glob.glob(os.path.join(d, "*.npz"))):
            with np.load(f) as z:
                for k in z.files:
                    assert k not in merged, "recorded twice: " + k
                    merged[k] = z[k]
    out = os.path.join(HERE, "ref_recordings.npz")
    np.savez_compressed(out, **merged)
    print("wrote %s: %d arrays, %d bytes" % (out, len(merged), os.path.getsize(out)))


if __name__ == "__main__":
    main()
