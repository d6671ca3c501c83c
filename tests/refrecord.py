"""Recorded results of the compiled reference (oracle/_ref) for the differential tests, so that they need nothing outside the
repository: where the reference is not built the tests compare against tests/golden/ref_<name>.json.gz instead of the live module.

    BSQ_RECORD_REF=1 python -m pytest tests/test_flatfile.py tests/test_oracle_golden.py tests/test_oracle_properties.py -m "not gpu"

(with oracle/_ref built) rewrites the records from the reference itself."""
import gzip
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def recording():
    return os.environ.get("BSQ_RECORD_REF") == "1"


def digest(*items):
    """one short hash over arrays (dtype, shape, bytes) and bytes / str"""
    h = hashlib.sha256()
    for a in items:
        if isinstance(a, np.ndarray):
            h.update(("%s%r" % (a.dtype.str, a.shape)).encode())
            a = np.ascontiguousarray(a).tobytes()
        elif isinstance(a, str):
            a = a.encode()
        h.update(len(a).to_bytes(8, "little"))
        h.update(a)
    return h.hexdigest()[:24]


class Record:
    """An ordered list of [key, value] pairs.  Recording: `see` appends the reference's value.  Otherwise: `see` checks that the
    next recorded key is this one (the test generated the same inputs) and that the value equals the recorded one."""

    def __init__(self, name):
        self.path = os.path.join(GOLDEN, "ref_%s.json.gz" % name)
        self.rec = recording()
        if self.rec:
            self.items = []
        else:
            with gzip.open(self.path, "rt") as f:
                self.items = json.load(f)
        self.i = 0

    def see(self, key, value):
        if self.rec:
            self.items.append([key, value])
            return
        assert self.i < len(self.items), ("more results than %s recorded" % os.path.basename(self.path), key)
        k, v = self.items[self.i]
        self.i += 1
        assert k == key, ("the test's inputs differ from those %s was recorded on" % os.path.basename(self.path), key, k)
        assert v == value, (key, "reference (recorded):", v, "got:", value)

    def close(self):
        if self.rec:
            with gzip.GzipFile(self.path, "wb", mtime=0) as f:
                f.write(json.dumps(self.items, separators=(",", ":")).encode())
        else:
            assert self.i == len(self.items), ("fewer results than %s recorded" % os.path.basename(self.path), self.i, len(self.items))
