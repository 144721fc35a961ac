"""The container files under tests/golden/containers/, without a GPU:
save_packed / save_tiled / save_set of the tensors the generator there builds
write exactly the committed bytes, and load_* of every committed file returns
those tensors (tests/golden/containers/make_containers.py)."""
import dataclasses
import importlib.util
import os

import pytest

from conftest import ROOT

DIR = os.path.join(ROOT, "tests", "golden", "containers")
NAMES = ["batch.nicepack", "image_v1.nicetile", "image_v2.nicetile", "set_v1.nicesets", "set_v2.nicesets"]


@pytest.fixture(scope="module")
def cases(nice):
    import torch
    spec = importlib.util.spec_from_file_location("make_containers", os.path.join(DIR, "make_containers.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    got = gen.cases(nice, torch)
    assert sorted(got) == sorted(NAMES)
    return got


def _same(torch, a, b):
    """Field by field: tensors by dtype, device and value, the rest by ==."""
    if dataclasses.is_dataclass(a):
        a, b = dataclasses.astuple(a), dataclasses.astuple(b)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            _same(torch, x, y)
        elif hasattr(x, "dtype"):
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y)
        else:
            assert x == y and type(x) is type(y)


@pytest.mark.parametrize("name", NAMES)
def test_save_writes_the_golden_bytes(cases, tmp_path, name):
    save, _, obj = cases[name]
    path = str(tmp_path / name)
    save(path, obj)
    want = open(os.path.join(DIR, name), "rb").read()
    assert 100 < len(want) < 1000
    assert open(path, "rb").read() == want


@pytest.mark.parametrize("name", NAMES)
def test_load_returns_the_tables(cases, name):
    import torch
    _, load, obj = cases[name]
    got = load(os.path.join(DIR, name))
    if name.endswith("_v2.nicetile") or name.endswith("_v2.nicesets"):
        assert got.alpha is not None and set(got.alpha.kind.tolist()) == {0, 1, 2}
    _same(torch, got, obj)
