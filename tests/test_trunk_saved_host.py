"""trunk._save / trunk._saved: the one pack / unpack pair for what the fused nodes' backwards keep (host tensors, a stand-in ctx)."""
import pytest
import torch

from gnn_tail_generalization_amd import trunk

ORDER = ('xd', 'x0', 'w_in', 'w_out', 'saved_in', 'saved_bits', 'layer_params', 'h_last', 'h_below', 'x0_bits')      # as trunk._save documents it


class _Ctx:
    """What _save / _saved touch of an autograd ctx: save_for_backward stores its arguments, saved_tensors hands them back."""

    def save_for_backward(self, *tensors):
        assert not hasattr(self, 'saved_tensors'), 'save_for_backward is called once'
        self.saved_tensors = tensors


def _t():
    return torch.zeros(2)


def _flatten(named):
    """The non-None tensors of `named` in ORDER, lists in their own order."""
    flat = []
    for name in ORDER:
        v = named[name]
        flat += [t for t in v if t is not None] if isinstance(v, (list, tuple)) else [v] if v is not None else []
    return flat


@pytest.mark.parametrize('les', [(False, False, False), (True, True, True), (True, False, True), (False, True, False)])
@pytest.mark.parametrize('h_last', [False, True])
@pytest.mark.parametrize('h_below', [False, True])
@pytest.mark.parametrize('x0_bits', [False, True])
@pytest.mark.parametrize('absent_in', [(), (0,), (2,), (1, 2)])
def test_saved_tensors_come_back_by_name(les, h_last, h_below, x0_bits, absent_in):
    L = len(les)
    layer_params = []
    for has_le in les:
        layer_params += [_t(), _t(), _t() if has_le else None]
    named = dict(xd=_t(), x0=_t(), w_in=_t(), w_out=_t(),
                 saved_in=[None if l in absent_in else _t() for l in range(L + 1)], saved_bits=[_t() for _ in range(L)],
                 layer_params=tuple(layer_params), h_last=_t() if h_last else None, h_below=_t() if h_below else None,
                 x0_bits=_t() if x0_bits else None)
    assert tuple(named) == ORDER
    ctx = _Ctx()
    trunk._save(ctx, **named)
    # the flat tuple: tensors only, in the documented order
    flat = ctx.saved_tensors
    assert all(isinstance(t, torch.Tensor) for t in flat)
    want = _flatten(named)
    assert len(flat) == len(want) and all(a is b for a, b in zip(flat, want))
    # every name comes back as the same object, or None
    back = trunk._saved(ctx)
    assert tuple(back) == ORDER
    for name, v in named.items():
        if isinstance(v, (list, tuple)):
            assert len(back[name]) == len(v) and all(a is b for a, b in zip(back[name], v)), name
        else:
            assert back[name] is v, name
    # ... and the per-layer (w, b, le) are re-formed from them
    lp = trunk._layers(back['layer_params'])
    assert len(lp) == L and all(lp[l][k] is layer_params[3 * l + k] for l in range(L) for k in range(3))


def test_stack_layout():
    """stack.py keeps saved_in, saved_bits and the layer parameters alone: the same pair, its own names."""
    named = dict(saved_in=[_t(), _t()], saved_bits=[_t()], layer_params=(_t(), _t(), None, _t(), _t(), _t()))
    ctx = _Ctx()
    trunk._save(ctx, **named)
    assert len(ctx.saved_tensors) == 8 and all(isinstance(t, torch.Tensor) for t in ctx.saved_tensors)
    back = trunk._saved(ctx)
    assert back['layer_params'][2] is None and back['layer_params'][5] is named['layer_params'][5] and back['saved_in'][1] is named['saved_in'][1]
