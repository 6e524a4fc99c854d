import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "midvision-probe_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_sessionstart(session):
    """A fresh checkout has no libmvp_hip.so (built artefacts are git-ignored): build it once (hipcc cross-compiles gfx950
    without a GPU) so that the ABI tests can load it.  An existing library is left alone."""
    so = os.path.join(PKG, "csrc", "libmvp_hip.so")
    if not os.path.exists(so):
        import subprocess

        subprocess.run(["make", "-C", os.path.join(PKG, "csrc")], check=False, stdout=subprocess.DEVNULL)


class Golden(dict):
    """The arrays of one fixture, by name (``.files`` lists them in stored order, as ``np.load`` of an .npz does)."""

    @property
    def files(self):
        return list(self)


def load_golden(name):
    """tests/golden/<name> together with its continuation files <stem>.part1.npz, <stem>.part2.npz, ... and arrays stored in
    row blocks ``<key>::chunk<i>`` joined back along axis 0: make_goldens.save_golden splits a fixture so that no committed file
    exceeds 1 MiB."""
    stem = os.path.splitext(name)[0]
    paths = [os.path.join(GOLDEN, name)]
    i = 1
    while os.path.exists(os.path.join(GOLDEN, f"{stem}.part{i}.npz")):
        paths.append(os.path.join(GOLDEN, f"{stem}.part{i}.npz"))
        i += 1
    g, chunks = Golden(), {}
    for p in paths:
        with np.load(p, allow_pickle=False) as z:
            for k in z.files:
                key, sep, _ = k.partition("::chunk")
                if sep:
                    g.setdefault(key, None)  # (keeps the array's place in the stored order)
                    chunks.setdefault(key, []).append(z[k])
                else:
                    g[k] = z[k]
    for key, parts in chunks.items():
        g[key] = np.concatenate(parts, axis=0)
    return g


@pytest.fixture(scope="session")
def golden():
    return load_golden


def rel_l2(a, b):
    """Relative L2 error ||a-b|| / ||b|| in float64 (the "rel" of north_star's 1e-3)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def max_rel(a, b):
    """max |a-b| / max |b|."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
