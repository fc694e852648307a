#!/usr/bin/env python
"""Record the reference's side of tests/test_host_logic.py and tests/test_writers.py into
tests/golden/host_logic_reference.pt.gz and tests/golden/writers_reference.pt.gz (tests/refgolden.py).

Runs both test modules with WHISPER_AMD_RECORD_REFERENCE=1: every `expect(...)` then evaluates its lambda against the
live reference (openai/whisper, imported from the checkout given here, beside the tokenizer shims of tests/shims), the
test's assertions compare this package with those fresh values, and the values are written at the end.  CPU only.

    python tests/golden/make_golden_host.py <path of an openai/whisper checkout>
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "whisper")):
        raise SystemExit(__doc__)
    env = dict(os.environ, WHISPER_AMD_RECORD_REFERENCE="1", WHISPER_AMD_REFERENCE=os.path.abspath(sys.argv[1]))
    subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                    os.path.join("tests", "test_host_logic.py"), os.path.join("tests", "test_writers.py")],
                   cwd=ROOT, env=env, check=True)


if __name__ == "__main__":
    main()
