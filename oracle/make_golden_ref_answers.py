"""Recorded answers of the UNMODIFIED reference (TEST INFRASTRUCTURE): every ref().encode / ref().decode call the tests below make,
answered by oracle/_ref/libfpng_ref.so and kept as size or status + dimensions + a digest of the bytes (tests/cpu_ref.py
_RecordingRef).  On a checkout without the reference build those tests are judged by these answers (tests/cpu_ref.py _RecordedRef).

Run where the reference build is present (after __graft_entry__.build()):   python oracle/make_golden_ref_answers.py
Writes tests/golden/ref_answers.npz (rewritten from scratch); the tests must pass while it is recorded."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = [
    "tests/test_oracle.py::test_oracle_vs_reference_fuzz",
    "tests/test_oracle.py::test_oracle_vs_reference_adjust_freq_quirk",
    "tests/test_oracle.py::test_reference_decodes_oracle_output",
    "tests/test_oracle.py::test_oracle_vs_reference_wide_rows",
    "tests/test_oracle.py::test_oracle_vs_reference_at_the_stored_or_compressed_boundary",
    "tests/test_oracle.py::test_oracle_vs_reference_on_skewed_histograms",
    "tests/test_dropin_decode.py::test_status_codes_match_reference_on_damaged_files",
    "tests/test_dropin_decode.py::test_container_and_block_edits_get_the_references_answer",
    "tests/test_dropin_decode.py::test_other_huffman_tables_and_the_reserved_length_symbols",
    "tests/test_dropin_decode.py::test_flat_rows_with_a_run_at_the_first_pixel",
    "tests/test_decode_model.py::test_edited_token_streams_get_the_references_answer",
    "tests/test_decode_model.py::test_edited_token_streams_of_megapixel_images",
    "tests/test_sync_cases_cpu.py::test_case_is_valid_and_shows_its_property",
    "tests/test_sync_cases_cpu.py::test_batch_is_valid_and_shows_its_property",
]


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cpu_ref
    if not cpu_ref.have_ref():
        raise SystemExit("oracle/_ref/libfpng_ref.so is not built: the reference's sources are needed to record its answers")
    if os.path.exists(cpu_ref.ANSWERS):
        os.remove(cpu_ref.ANSWERS)
    # one pytest process per test file: each one merges what it recorded into the file when it ends
    for f in sorted({t.split("::")[0] for t in TESTS}):
        ids = [t for t in TESTS if t.startswith(f + "::")]
        subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", *ids], cwd=ROOT,
                              env=dict(os.environ, FPNG_RECORD_REF_ANSWERS="1"))
    print("wrote", cpu_ref.ANSWERS, os.path.getsize(cpu_ref.ANSWERS), "bytes")


if __name__ == "__main__":
    main()
