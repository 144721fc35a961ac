"""Refusals the Python layer raises itself on the tiled and set paths, before
(colour tables, outputs, arguments) or between (alpha tables) the library
calls: every one is NiceError(E_ARG).  A colour-table refusal comes before any
launch, so the outputs, pre-filled with a poison byte, stay untouched; an
alpha-table refusal comes after the colour pass, so nothing is asserted about
the output there.

One RGBA image of 40 x 24 at 16 x 16 tiles (3 x 2 tiles), and the set of that
image and a 17 x 9 one (8 tiles), both encoded with alpha=True."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG = -1
POISON = 0xA5
TILE = (16, 16)
N_TILED, N_SET = 6, 8


@pytest.fixture(scope="module")
def ctx(nice):
    return nice.Context(0)


@pytest.fixture(scope="module")
def images(O):
    import torch
    out = []
    for w, h, seed in ((40, 24, 11), (17, 9, 12)):
        px = O.gen_syn_v1(w, h, 4, seed).reshape(h, w, 4).copy()
        px[:, :, 3] = np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)
        out.append(torch.from_numpy(px).cuda())
    return out


@pytest.fixture(scope="module")
def timg(nice, ctx, images):
    t = nice.encode_tiled(images[0], tile=TILE, ctx=ctx, alpha=True)
    assert t.nx * t.ny == N_TILED and t.alpha is not None and t.nbytes >= 16 and t.alpha.nbytes >= 16
    return t


@pytest.fixture(scope="module")
def iset(nice, ctx, images):
    s = nice.encode_set(images, tile=TILE, ctx=ctx, alpha=True)
    assert s.first == [0, 6, N_SET] and s.alpha is not None and s.nbytes >= 16 and s.alpha.nbytes >= 16
    return s


def _poisoned(torch, *shape, dtype=None):
    t = torch.empty(shape, dtype=torch.uint8 if dtype is None else dtype, device="cuda")
    t.view(torch.uint8).fill_(POISON)
    return t


def _untouched(torch, outs):
    return all(bool((o.contiguous().view(torch.uint8) == POISON).all()) for o in outs)


def _refused(nice, fn, *a, **kw):
    with pytest.raises(nice.NiceError) as e:
        fn(*a, **kw)
    assert e.value.code == E_ARG, (a, kw)


def _broken_tables(obj, n):
    """The five colour-table faults, each as a copy of ``obj``."""
    return {"packed on the CPU": dataclasses.replace(obj, packed=obj.packed.cpu()),
            "stream_len short": dataclasses.replace(obj, stream_len=obj.stream_len[:-1]),
            "kind short": dataclasses.replace(obj, kind=obj.kind[:-1]),
            "off of n entries": dataclasses.replace(obj, off=obj.off[:n]),
            "off[n] past packed": dataclasses.replace(obj, packed=obj.packed[:-16])}


def _broken_alpha(obj, n):
    """The three alpha-table faults, each as a copy of ``obj``."""
    al = obj.alpha
    return {"alpha.packed on the CPU": dataclasses.replace(obj, alpha=dataclasses.replace(al, packed=al.packed.cpu())),
            "alpha.value short": dataclasses.replace(obj, alpha=dataclasses.replace(al, value=al.value[:-1])),
            "alpha.off of n entries": dataclasses.replace(obj, alpha=dataclasses.replace(al, off=al.off[:n]))}


@pytest.mark.parametrize("oc", [3, 4])
def test_decode_tiled_colour_tables(nice, ctx, timg, oc):
    import torch
    for why, t in _broken_tables(timg, N_TILED).items():
        out = _poisoned(torch, 24, 40, oc)
        _refused(nice, nice.decode_tiled, t, out=out, ctx=ctx)
        torch.cuda.synchronize()
        assert _untouched(torch, [out]), why
        _refused(nice, nice.decode_tiled, t, roi=(3, 2, 20, 17), ctx=ctx)


@pytest.mark.parametrize("oc", [3, 4])
def test_decode_set_colour_tables(nice, ctx, iset, oc):
    import torch
    for why, s in _broken_tables(iset, N_SET).items():
        outs = [_poisoned(torch, 24, 40, oc), _poisoned(torch, 9, 17, oc)]
        _refused(nice, nice.decode_set, s, out=outs, ctx=ctx)
        crops = _poisoned(torch, 2, 8, 9, oc)
        _refused(nice, nice.decode_set, s, windows=[(0, 30, 10, 9, 8), (1, 8, 1, 9, 8)], out=crops, ctx=ctx)
        torch.cuda.synchronize()
        assert _untouched(torch, outs + [crops]), why
        _refused(nice, nice.decode_set, s, images=[1], ctx=ctx)


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_decode_set_tensor_colour_tables(nice, ctx, iset, dtype):
    import torch
    dt = getattr(torch, dtype)
    for why, s in _broken_tables(iset, N_SET).items():
        outs = [_poisoned(torch, 3, 24, 40, dtype=dt), _poisoned(torch, 3, 9, 17, dtype=dt)]
        _refused(nice, nice.decode_set_tensor, s, out=outs, dtype=dt, ctx=ctx)
        crops = _poisoned(torch, 2, 3, 8, 9, dtype=dt)
        _refused(nice, nice.decode_set_tensor, s, windows=[(0, 30, 10, 9, 8), (1, 8, 1, 9, 8)], out=crops, dtype=dt,
                 ctx=ctx)
        torch.cuda.synchronize()
        assert _untouched(torch, outs + [crops]), why
        _refused(nice, nice.decode_set_tensor, s, images=[1], dtype=dt, ctx=ctx)


def test_alpha_tables(nice, ctx, timg, iset):
    """Refused after the colour pass (the output is not looked at); with three
    output channels the alpha batch is not read and the same objects decode."""
    import torch
    for t in _broken_alpha(timg, N_TILED).values():
        _refused(nice, nice.decode_tiled, t, ctx=ctx)
        _refused(nice, nice.decode_tiled, t, roi=(3, 2, 20, 17), out_channels=4, ctx=ctx)
        assert tuple(nice.decode_tiled(t, out_channels=3, ctx=ctx).shape) == (24, 40, 3)
    for s in _broken_alpha(iset, N_SET).values():
        _refused(nice, nice.decode_set, s, ctx=ctx)
        _refused(nice, nice.decode_set, s, windows=[(1, 8, 1, 9, 8)], out_channels=4, ctx=ctx)
        assert [tuple(o.shape) for o in nice.decode_set(s, out_channels=3, ctx=ctx)] == [(24, 40, 3), (9, 17, 3)]
    torch.cuda.synchronize()


def test_decode_tiled_outputs(nice, ctx, timg):
    import torch
    for shape in ((24, 41, 4), (25, 40, 4), (24, 40), (1, 24, 40, 4)):
        _refused(nice, nice.decode_tiled, timg, out=_poisoned(torch, *shape), ctx=ctx)
    _refused(nice, nice.decode_tiled, timg, roi=(0, 0, 20, 17), out=_poisoned(torch, 24, 40, 4), ctx=ctx)
    out = _poisoned(torch, 24, 40, 4)
    _refused(nice, nice.decode_tiled, timg, out=out, out_channels=3, ctx=ctx)      # contradicts out
    out3 = _poisoned(torch, 24, 40, 3)
    _refused(nice, nice.decode_tiled, timg, out=out3, out_channels=4, ctx=ctx)
    _refused(nice, nice.decode_tiled, timg, out=torch.full((24, 40, 4), POISON, dtype=torch.uint8), ctx=ctx)   # CPU
    torch.cuda.synchronize()
    assert _untouched(torch, [out, out3])


def test_encode_set_arguments(nice, ctx, images):
    _refused(nice, nice.encode_set, [], tile=TILE, ctx=ctx)
    _refused(nice, nice.encode_set, iter(()), tile=TILE, ctx=ctx)
    rgb = images[1][:, :, :3].contiguous()
    _refused(nice, nice.encode_set, [images[0], rgb], tile=TILE, ctx=ctx)          # 4 and 3 channels together
    _refused(nice, nice.encode_set, [rgb, images[0]], tile=TILE, ctx=ctx)
    _refused(nice, nice.encode_set, [rgb], tile=TILE, ctx=ctx, alpha=True)         # alpha of a 3-channel set
    _refused(nice, nice.encode_tiled, rgb, tile=TILE, ctx=ctx, alpha=True)


def test_decode_set_tensor_arguments(nice, ctx, iset):
    """What tests/test_sets_tensor.py::test_rejects leaves out: bias of the
    wrong length, a negative image index, a window that is not a quintuple,
    and a list of outputs one of which is no tensor, has another window's
    shape, another dtype or lies on the CPU."""
    import torch
    f16 = torch.float16
    _refused(nice, nice.decode_set_tensor, iset, bias=(0, 0), ctx=ctx)
    _refused(nice, nice.decode_set_tensor, iset, bias=(0, 0, 0, 0), ctx=ctx)
    _refused(nice, nice.decode_set_tensor, iset, scale=(1, 1, 1, 1), ctx=ctx)
    _refused(nice, nice.decode_set_tensor, iset, images=[-1], ctx=ctx)
    _refused(nice, nice.decode_set_tensor, iset, images=[2], ctx=ctx)
    _refused(nice, nice.decode_set_tensor, iset, windows=[(0, 0, 0, 9)], ctx=ctx)
    _refused(nice, nice.decode_set_tensor, iset, windows=[(0, 0, 0, 9, 8, 1)], ctx=ctx)
    good = [_poisoned(torch, 3, 24, 40, dtype=f16), _poisoned(torch, 3, 9, 17, dtype=f16)]
    for second in (None, _poisoned(torch, 3, 24, 40, dtype=f16), _poisoned(torch, 3, 9, 17, dtype=torch.float32),
                   torch.empty((3, 9, 17), dtype=f16), _poisoned(torch, 9, 17, 3, dtype=f16)):
        _refused(nice, nice.decode_set_tensor, iset, out=[good[0], second], ctx=ctx)
    _refused(nice, nice.decode_set_tensor, iset, out=good + good[1:], ctx=ctx)
    _refused(nice, nice.decode_set_tensor, iset, out=good, flip=[0], ctx=ctx)
    torch.cuda.synchronize()
    assert _untouched(torch, good)
    # the same refusals on decode_set
    _refused(nice, nice.decode_set, iset, images=[-1], ctx=ctx)
    _refused(nice, nice.decode_set, iset, images=[0], windows=[(0, 0, 0, 9, 8)], ctx=ctx)
    _refused(nice, nice.decode_set, iset, windows=[(0, 0, 0, 9)], ctx=ctx)
    _refused(nice, nice.decode_set, iset, out=[_poisoned(torch, 24, 40, 4)], ctx=ctx)
    _refused(nice, nice.decode_set, iset, out=_poisoned(torch, 3, 24, 40, 4), ctx=ctx)
    _refused(nice, nice.decode_set, iset, out=[_poisoned(torch, 24, 40, 4), _poisoned(torch, 9, 17, 3)], ctx=ctx)
    _refused(nice, nice.decode_set, iset, out=[_poisoned(torch, 24, 40, 4), _poisoned(torch, 9, 17, 4)], out_channels=3,
             ctx=ctx)
