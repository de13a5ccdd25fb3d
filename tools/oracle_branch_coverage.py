"""Which encoder branches of the oracle does the encoder corpus leave untaken?  CPU only.

Builds oracle/flac_oracle.c with --coverage into a temporary directory, runs every case of tests/encoder_corpus.py through
that build (encode and decision trace, in a child process so that the counters are written when it exits), and prints
the branches of the encoder -- rice_search through encode_frame -- that were never taken, with their source lines.
tests/encoder_corpus.py's docstring argues why each of them is unreachable; profiles/encoder_corpus.md keeps the output.

    python tools/oracle_branch_coverage.py [--histogram]

--histogram also prints how often the corpus reaches each decision of tests/test_encoder_corpus.py's table.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "oracle", "flac_oracle.c")

CHILD = """
import sys
sys.path.insert(0, {root!r})
from oracle import oracle as O
O._LIB = O.load({so!r})
from tests import encoder_corpus as C
for c in C.CASES:
    (O.encode_i64 if c.is_int64 else O.encode_i32)(c.x, c.level)
    C.trace_case(O, c)
    (O.stream_info_i64 if c.is_int64 else O.stream_info)(c.x[0], c.level)
"""


def encoder_lines():
    """[first, last] source lines of rice_search .. encode_frame"""
    first = last = None
    with open(SRC) as f:
        for no, line in enumerate(f, 1):
            if line.startswith("static bool rice_search("):
                first = no
            if line.startswith("static int64_t stream_header_bytes("):
                last = no - 1
    assert first and last and first < last
    return first, last


def untaken(gcov_text, first, last):
    out, src_no, src = [], 0, ""
    for line in gcov_text.splitlines():
        m = re.match(r"\s*([-#=\d*]+):\s*(\d+):(.*)$", line)
        if m:
            src_no, src = int(m.group(2)), m.group(3).strip()
            continue
        m = re.match(r"branch\s+(\d+)\s+(never executed|taken (\d+))", line)
        if m and first <= src_no <= last and (m.group(2) == "never executed" or int(m.group(3)) == 0):
            out.append((src_no, int(m.group(1)), m.group(2), src))
    return out


def main():
    first, last = encoder_lines()
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "liboracle_cov.so")
        subprocess.check_call(["gcc", "-O0", "-g", "--coverage", "-std=c11", "-fPIC", "-mfma", "-ffp-contract=off", "-c", "-o", "flac_oracle.o", SRC], cwd=tmp)
        subprocess.check_call(["gcc", "--coverage", "-shared", "-o", so, "flac_oracle.o", "-lm"], cwd=tmp)
        subprocess.check_call([sys.executable, "-c", CHILD.format(root=ROOT, so=so)], cwd=tmp)
        subprocess.check_call(["gcov", "-b", "-c", "-o", tmp, SRC], cwd=tmp, stdout=subprocess.DEVNULL)
        with open(os.path.join(tmp, "flac_oracle.c.gcov")) as f:
            text = f.read()
    rows = untaken(text, first, last)
    print(f"untaken encoder branches (flac_oracle.c lines {first}-{last}, corpus of {_n_cases()} cases): {len(rows)}")
    for no, br, how, src in rows:
        print(f"  line {no} branch {br} ({how}): {src}")
    if "--histogram" in sys.argv:
        histogram()


def _n_cases():
    sys.path.insert(0, ROOT)
    from tests import encoder_corpus as C

    return len(C.CASES)


def histogram():
    sys.path.insert(0, ROOT)
    from oracle import oracle as O

    O.build()
    from tests import encoder_corpus as C
    from tests.test_encoder_corpus import DECISIONS

    recs = [r for c in C.CASES for r in C.trace_case(O, c)]
    print(f"decision histogram ({len(recs)} subframes):")
    for d, pred in DECISIONS.items():
        print(f"  {d}: {sum(1 for r in recs if pred(r))}")


if __name__ == "__main__":
    main()
