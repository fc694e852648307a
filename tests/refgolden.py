"""Stored answers of the reference (openai/whisper) for the tests that compare this package with it.

A test wraps every reference-side expression in `expect(lambda: ...)`.  Normally the value comes from
tests/golden/<name>.pt.gz; with WHISPER_AMD_RECORD_REFERENCE=1 and the reference checkout on the path given by
WHISPER_AMD_REFERENCE (tests/golden/make_golden_host.py sets both) the lambda runs against the live reference and its
value is stored.  Either way the test's own assertions run on the value.  Values are plain data (tensors, lists, tuples,
dicts, str, numbers): they load with torch.load(weights_only=True)."""
import copy
import gzip
import io
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SHIMS = os.path.join(HERE, "shims")
RECORD = os.environ.get("WHISPER_AMD_RECORD_REFERENCE") == "1"


def live_reference():
    """the reference package itself (recording only)"""
    root = os.environ.get("WHISPER_AMD_REFERENCE", "")
    if not os.path.isdir(os.path.join(root, "whisper")):
        raise RuntimeError("WHISPER_AMD_RECORD_REFERENCE=1 needs WHISPER_AMD_REFERENCE=<reference checkout>")
    for p in (SHIMS, root):
        if p not in sys.path:
            sys.path.insert(0, p)
    import whisper
    import whisper.decoding
    import whisper.timing
    import whisper.tokenizer
    import whisper.utils
    return whisper


class Store:
    def __init__(self, name):
        self.path = os.path.join(GOLDEN, f"{name}.pt.gz")
        self.ref = live_reference() if RECORD else None
        if RECORD:
            self.data = {}
        else:
            with gzip.open(self.path, "rb") as f:
                self.data = torch.load(io.BytesIO(f.read()), weights_only=True)

    def save(self):
        buf = io.BytesIO()
        torch.save(self.data, buf)
        with gzip.GzipFile(self.path, "wb", mtime=0) as f:
            f.write(buf.getvalue())

    def expect_for(self, test):
        """the `expect` of one test: its n-th call returns the n-th stored answer of that test"""
        counter = iter(range(1 << 30))

        def expect(fn):
            key = f"{test}/{next(counter)}"
            if RECORD:
                self.data[key] = fn()
            assert key in self.data, f"no stored reference answer {key}: regenerate with tests/golden/make_golden_host.py"
            return copy.deepcopy(self.data[key])           # the test may edit what it gets; the stored answer stays
        return expect


def store_fixture(name):
    """module-scoped fixture: the Store of `name`, written back at the end of a recording run"""
    @pytest.fixture(scope="module")
    def _store():
        s = Store(name)
        yield s
        if RECORD:
            s.save()
    return _store


def raises(exc, fn):
    """what the reference does on bad input, as data: the exception's type name and message, or None"""
    try:
        fn()
    except exc as e:        # noqa: PERF203
        return (type(e).__name__, str(e))
    return None
