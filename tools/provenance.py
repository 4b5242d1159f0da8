"""Hashes that tie a committed measurement / parity record to the sources it was made with (bench.py and the parity tools stamp
their records with them and refuse to quote a record whose hash differs from the working tree)."""
import hashlib
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lt-mapper_amd", "csrc")
# Listed from the directory, not by hand: a new kernel unit, C ABI unit or shared header is hashed without anyone having to remember it.
_API_HEADERS = ("ltm_internal.h", "ltm_pclsort.h")
_ALL = sorted(os.listdir(CSRC))
KERNEL_SOURCES = tuple(f for f in _ALL if (f.startswith("ltm_k_") and f.endswith(".hip")) or (f.endswith(".h") and f not in _API_HEADERS))
API_SOURCES = tuple(f for f in _ALL if (f.startswith("ltm_api_") and f.endswith(".cpp")) or f in _API_HEADERS)


def _sha(files):
    h = hashlib.sha256()
    for f in files:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()[:16]


def kernels_sha():
    """the device code: what the PMC / rocprof figures of a kernel depend on"""
    return _sha(KERNEL_SOURCES)


def product_sha():
    """device code + the C ABI orchestration: what the RESULTS of the library depend on"""
    return _sha(KERNEL_SOURCES + API_SOURCES)


def oracle_sha():
    h = hashlib.sha256()
    for f in ("ltm_oracle.cpp", "oracle_math.h", "ltm_oracle.h"):
        h.update(open(os.path.join(ROOT, "oracle", f), "rb").read())
    return h.hexdigest()[:16]
