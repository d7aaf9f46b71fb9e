"""CPU: frozen parameters (requires_grad=False) in the fused train step -- the host side.  The span table the optimiser kernels take, the
backward plan (which weight-gradient products run, where the pass stops), the exchange layout, the no-trainable-parameter error, the
data-parallel agreement check over gloo, and the resources of the two span kernels."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd.engine import BackwardPlan, VitEngine
from ecg_representation_learning_amd.train import span_table, trainable_ranges

CONF = dict(max_signal_length=400, patch_size=20, hidden_size=64, num_hidden_layers=4, num_attention_heads=2, intermediate_size=128)
LINEARS = ('0.fn.to_qkv.weight', '0.fn.to_out.0.weight', '1.fn.net.0.weight', '1.fn.net.3.weight')


def _model(masked=False):
    m = E.EcgVit(config=E.EcgVitConfig(**CONF))
    return E.MaskedEcgVit(m).encoder if masked else m


def freeze(model, trainable):
    """requires_grad = trainable(name) for every parameter of the flat layout"""
    for n, p in zip(model._param_names, model._param_list):
        p.requires_grad_(bool(trainable(n)))
    return [n for n, p in zip(model._param_names, model._param_list) if p.requires_grad]


def linear_probe(n):
    return n.startswith('vit.mlp_head.')


def top_blocks(k, ly):
    return lambda n: n.startswith('vit.mlp_head.') or any(n.startswith(f'vit.transformer.layers.{i}.') for i in range(ly - k, ly))


def bitfit(n):
    return n.endswith('.bias')


def _flags(model):
    return [p.requires_grad for p in model._param_list]


def test_span_table_from_flags():
    m = _model()
    lay, names = m._layout, m._param_names
    lag = [0] * len(names)
    assert span_table(lay, names, [True] * len(names), lag) is None
    # linear probe: the head is one contiguous run at the end of the layout
    freeze(m, linear_probe)
    rows = span_table(lay, names, _flags(m), lag)
    lo = lay.entries['vit.mlp_head.0.weight'][0]
    off, _, n = lay.entries['vit.mlp_head.1.bias']
    assert rows == [[lo, off + n - lo, 0]]
    # top 2 blocks + head: one run from block 2 to the head
    freeze(m, top_blocks(2, 4))
    rows = span_table(lay, names, _flags(m), lag)
    lo = min(o for k, (o, _, _) in lay.entries.items() if k.startswith('vit.transformer.layers.2.'))
    assert rows == [[lo, off + n - lo, 0]]
    # BitFit: no two biases are neighbours in the layout, so every bias is a span of its own
    tr = freeze(m, bitfit)
    rows = span_table(lay, names, _flags(m), lag)
    covered = set()
    for o, c, s in rows:
        assert s == 0
        covered |= {k for k, (oo, _, cc) in lay.entries.items() if o <= oo and oo + cc <= o + c}
    assert covered == set(tr)
    assert len(rows) == len(tr) == 1 + 5 * 4 + 2   # patch bias, 5 per block (to_qkv has none), the head's two
    assert len(rows) <= 100


def test_span_table_splits_on_step_offsets():
    """a parameter unfrozen later has its own step count: it never merges with neighbours at another step"""
    m = _model()
    lay, names = m._layout, m._param_names
    freeze(m, top_blocks(2, 4))
    lag = [0 if linear_probe(n) else -2 for n in names]   # the head trained 2 steps longer
    rows = span_table(lay, names, _flags(m), lag)
    assert [r[2] for r in rows] == [-2, 0]
    assert span_table(lay, names, [True] * len(names), lag) is not None   # all trainable, unequal counts: still the span kernels


def test_no_trainable_parameter_raises():
    m = _model()
    freeze(m, lambda n: False)
    with pytest.raises(ValueError):
        span_table(m._layout, m._param_names, _flags(m), [0] * len(_flags(m)))
    with pytest.raises(ValueError):
        BackwardPlan(m._param_names, 4, [])
    step = E.HipTrainStep(m, dict(n_step=10))
    with pytest.raises(ValueError, match='no trainable parameter'):   # before anything touches a device (this machine has none)
        step.step(torch.zeros(2, 12, 400), torch.zeros(2, 71))
    enc = _model(masked=True)
    freeze(enc, lambda n: False)
    with pytest.raises(ValueError, match='no trainable parameter'):
        E.HipTrainStep(enc, dict(n_step=10)).step(torch.zeros(2, 12, 400), torch.zeros(2, 71))


def test_backward_plan_linear_probe():
    m = _model()
    tr = freeze(m, linear_probe)
    p = BackwardPlan(m._param_names, 4, tr)
    assert p.depth == 0 and p.wgrad == frozenset() and p.live == {'head'}
    # masked objective: the head is outside it -- nothing below the reconstruction product runs
    enc = _model(masked=True)
    tr = freeze(enc, linear_probe)
    assert BackwardPlan(enc._param_names, 4, tr, masked=True).depth == -1


def test_backward_plan_top_blocks():
    m = _model()
    for k in (1, 2, 4):
        tr = freeze(m, top_blocks(k, 4))
        p = BackwardPlan(m._param_names, 4, tr)
        low = 4 - k
        # stops with the LayerNorm-1 backward of the lowest trainable block: no input gradient below it, no embedding backward
        assert p.depth == 1 + 7 * (4 - 1 - low) + 6
        assert p.reach(p.depth) and not p.reach(p.depth + 1)
        assert p.wgrad == {f'vit.transformer.layers.{i}.{s}' for i in range(low, 4) for s in LINEARS}
        assert p.live == {'head'} | {f'layer{i}' for i in range(low, 4)}
    # the top block's FFN only: the pass stops inside the block, after the FFN-down input gradient
    tr = freeze(m, lambda n: n.startswith('vit.transformer.layers.3.1.fn.'))
    p = BackwardPlan(m._param_names, 4, tr)
    assert p.depth == 1 and p.wgrad == {'vit.transformer.layers.3.1.fn.net.0.weight', 'vit.transformer.layers.3.1.fn.net.3.weight'}


def test_backward_plan_bitfit_and_embedding():
    m = _model()
    tr = freeze(m, bitfit)
    p = BackwardPlan(m._param_names, 4, tr)
    assert p.wgrad == frozenset()                      # no weight-gradient product at all
    assert p.depth == 1 + 7 * 4                        # the patch-embedding bias: down through the embedding backward
    tr = freeze(m, lambda n: n == 'vit.to_patch_embedding.1.weight')
    p = BackwardPlan(m._param_names, 4, tr)
    assert p.wgrad == {'vit.to_patch_embedding.1.weight'} and p.depth == 1 + 7 * 4 and p.live == {'embed'}


def test_engine_full_set_is_the_full_pass():
    """trainable = every parameter (or None) gives no plan: the launch sequence of the pass without frozen parameters"""
    m = _model()
    c = m.config
    eng = VitEngine(C=c.num_channels, L=c.max_signal_length, P=c.patch_size, d=c.hidden_size, h=c.num_attention_heads, f=c.intermediate_size,
                    Ly=c.num_hidden_layers, K=m.num_class, p_hidden=0.0, p_emb=0.0, dtype=torch.float32, layout=m._layout)
    eng._begin_plan(None, masked=False)
    assert eng._plan is None
    eng._begin_plan(list(m._param_names), masked=False)
    assert eng._plan is None
    eng._begin_plan(['vit.mlp_head.1.weight'], masked=False)
    assert eng._plan is not None and not eng._wants('vit.transformer.layers.0.0.fn.to_qkv.weight') and not eng._reach(1)


def test_exchange_layout_drops_frozen_buckets():
    m = _model()
    lay = m._layout
    buckets = lay.buckets_in_ready_order(4)
    tr = freeze(m, top_blocks(1, 4))
    r = dict(trainable_ranges(lay, buckets, tr))
    assert list(r) == ['head', 'layer3']
    assert r['layer3'] == dict(buckets)['layer3'] and r['head'] == dict(buckets)['head']
    tr = freeze(m, lambda n: n == 'vit.transformer.layers.1.0.norm.bias')
    r = dict(trainable_ranges(lay, buckets, tr))
    off, _, n = lay.entries['vit.transformer.layers.1.0.norm.bias']
    assert r == {'layer1': (off, (off + n + 15) // 16 * 16)}


def test_autograd_surface_reads_the_flags():
    m = _model()
    assert m.trainable_names() is None
    tr = freeze(m, linear_probe)
    assert m.trainable_names() == tr


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _agree_worker(rank, world, port, out_dir, same):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import ecg_representation_learning_amd as E_
    flags = [True] * 40 + [False] * 10
    if not same and rank == 1:
        flags[3] = False
    try:
        E_.ddp.check_same_frozen_set(flags)
        res = 'ok'
    except ValueError as e:
        res = 'ValueError: ' + str(e)
    # the group is still usable afterwards: every rank took part in the same single collective
    t = torch.ones(1)
    dist.all_reduce(t)
    with open(os.path.join(out_dir, f'agree{rank}.txt'), 'w') as f:
        f.write(f'{res}\n{float(t)}')
    dist.destroy_process_group()


@pytest.mark.parametrize('same', [False, True])
def test_ranks_must_agree_on_the_frozen_set(tmp_path, same):
    world = 2
    mp.spawn(_agree_worker, args=(world, _free_port(), str(tmp_path), same), nprocs=world, join=True, start_method='spawn')
    out = [open(os.path.join(tmp_path, f'agree{r}.txt')).read().split('\n') for r in range(world)]
    for res, tot in out:
        assert float(tot) == world
        if same:
            assert res == 'ok'
        else:
            assert res.startswith('ValueError') and 'frozen' in res


def test_span_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import code_objects
    if not os.path.exists(code_objects.READELF):
        pytest.skip('llvm-readelf not in this image')
    ks = code_objects.kernels(os.path.join(ROOT, 'ecg-representation-learning_amd', 'libecgvit_hip.so'))
    found = [n for n in ks if 'adamw_spans_kernel' in n or 'sumsq_spans_partial_kernel' in n]
    assert len(found) == 2, found
    for n in found:
        k = ks[n]
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
