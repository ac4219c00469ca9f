"""The Python surface of pertgnn._C is pinned: the set of exported callables
and, for each, the signature line of its pybind docstring (name, argument
names, types, defaults, return type) equal tests/c_surface.json.  CPU only:
the extension imports without a GPU."""
import json
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")

from pertgnn.ops.backend import ext, has_hip  # noqa: E402

pytestmark = pytest.mark.skipif(not has_hip(), reason="pertgnn._C is not built")

SURFACE = Path(__file__).with_name("c_surface.json")


def current_surface():
    C = ext()
    out = {}
    for name in dir(C):
        obj = getattr(C, name)
        if name.startswith("_") or not callable(obj):
            continue
        out[name] = (obj.__doc__ or "").strip().splitlines()[0]
    return out


def test_exported_names():
    want = json.loads(SURFACE.read_text())
    got = current_surface()
    assert sorted(got) == sorted(want), (
        f"missing: {sorted(set(want) - set(got))}, "
        f"new: {sorted(set(got) - set(want))}")


def test_signatures():
    want = json.loads(SURFACE.read_text())
    got = current_surface()
    diff = {n: (want[n], got[n]) for n in want if n in got and want[n] != got[n]}
    assert not diff, "\n".join(
        f"{n}:\n  pinned  {a}\n  current {b}" for n, (a, b) in diff.items())


if __name__ == "__main__":  # regenerate the pinned surface from this build
    SURFACE.write_text(json.dumps(current_surface(), indent=1, sort_keys=True)
                       + "\n")
