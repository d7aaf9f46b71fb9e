"""CPU, world_size 2 / 4 / 8, gloo: the N > 1 path's logic -- contiguous equal shards, one SUM all-reduce over the flat gradient
buffer, 1/world folded into the update, clip on the REDUCED gradient -- reproduces the single-process full-batch step.
The per-rank compute here is the CPU oracle (the HIP kernels need a GPU); what is under test is ecg_..._amd.ddp + the
flat layout, which are device-agnostic and are exactly what HipTrainStep calls on the GPU.
The world-2/4/8 test takes each shard's oracle backward in the test process and hands it to its rank: torch's autograd engine
initialises every device runtime on its first backward, so eight ranks each running one would each open the GPU of a GPU machine."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import Cfg, ROOT


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


CFG = dict(max_signal_length=400, patch_size=20, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64)


def _global_batch(world):
    return 8 if world <= 4 else 16                      # global batch: 4 / 2 / 2 records per rank


def _shard_backward(world, out_dir):
    """each rank's forward + backward on ITS shard of the global batch, from rank 0's initial weights (seed 1234: what the broadcast hands
    every rank), taken here in the test process -> <out_dir>/shard<rank>.pt (loss, flat gradient)"""
    import ecg_representation_learning_amd as E
    from ecg_representation_learning_amd.engine import ParamLayout
    from oracle import vit_oracle as O
    G = _global_batch(world)
    x, y = O.synthetic_batch(G, length=400, seed=77)    # the GLOBAL batch
    for rank in range(world):
        torch.manual_seed(1234)
        model = O.OracleEcgVit(config=Cfg(**CFG)).train()
        layout = ParamLayout([(n, tuple(p.shape)) for n, p in model.named_parameters()])
        lo, hi = E.ddp.shard_range(G, rank, world)
        out = model(sample_values=x[lo:hi], labels=y[lo:hi])
        out.loss.backward()
        gflat = torch.zeros(layout.total)
        for n, p in model.named_parameters():
            layout.view(gflat, n).copy_(p.grad)
        torch.save(dict(loss=out.loss.detach(), g=gflat, lo=lo, hi=hi), os.path.join(out_dir, f'shard{rank}.pt'))


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import ecg_representation_learning_amd as E
    from ecg_representation_learning_amd.engine import ParamLayout
    from oracle import vit_oracle as O
    torch.set_num_threads(2 if world <= 2 else 1)
    torch.manual_seed(1234 + rank)                      # deliberately different init per rank ...
    model = O.OracleEcgVit(config=Cfg(**CFG)).train()
    layout = ParamLayout([(n, tuple(p.shape)) for n, p in model.named_parameters()])
    pflat = torch.zeros(layout.total)
    for n, p in model.named_parameters():
        layout.view(pflat, n).copy_(p.data)
        p.data = layout.view(pflat, n)
    E.ddp.broadcast_flat_(pflat, src=0)                 # ... made identical by one broadcast of the flat buffer
    shard = torch.load(os.path.join(out_dir, f'shard{rank}.pt'))   # this rank's shard backward, on rank 0's weights (_shard_backward)
    assert (shard['lo'], shard['hi']) == E.ddp.shard_range(_global_batch(world), rank, world)
    out_loss, gflat = shard['loss'], shard['g']
    cfg = Cfg(**CFG)
    # the train step's exchange object: per-layer buckets launched in backward order (overlap), f32 and bf16 on the wire
    local = gflat.clone()
    xout = {}
    for tag, kw in (('f32_overlap', dict(overlap=True)), ('f32_single', dict(overlap=False)),
                    ('bf16_overlap', dict(overlap=True, comm_dtype=torch.bfloat16)), ('bf16_single', dict(overlap=False, comm_dtype=torch.bfloat16))):
        g2 = local.clone()
        ranges = layout.buckets_in_ready_order(cfg.num_hidden_layers)
        ex = E.ddp.GradExchange(ranges, **kw)
        ex.begin(g2)
        for name, _ in ranges:
            ex.bucket_ready(name)
        ex.finish()
        xout[tag] = g2 / ex.world
    w = E.ddp.allreduce_flat_(gflat, bucket_elems=1000 if rank >= 0 else 0)   # bucketed variant
    gflat /= w
    norm = gflat.norm()
    coef = torch.clamp(1.0 / (norm + 1e-6), max=1.0)
    torch.save(dict(g=gflat * coef, norm=norm, loss=out_loss, p=pflat.clone(), seed=E.ddp.rank_seed(77, rank), xchg=xout, gavg=gflat.clone()),
               os.path.join(out_dir, f'rank{rank}.pt'))
    dist.all_reduce(torch.zeros(1))                     # every rank done before teardown (dist.barrier() would probe for, and open, a GPU)
    dist.destroy_process_group()


# bf16 on the wire: each rank's bucket is rounded to 8 significant bits and the ring sums in bf16 -> relative error of the reduced
# gradient ~2^-9 * sqrt(world).  Bounds per world size, and the bf16 path's own per-tensor gradient tolerance (cosine >= 0.98,
# tests/test_gpu_configs.py) held against the f32 exchange: measured here (gloo ring) 2.3e-3 / 2.7e-3 / 3.1e-3 at world 2 / 4 / 8, worst cosine 0.99999
# for every parameter tensor -- bf16 buckets stay a supported wire dtype at 8 ranks (f32 remains the default).
BF16_WIRE_REL = {2: 8e-3, 4: 1.0e-2, 8: 1.4e-2}


@pytest.mark.parametrize('world', [2, 4, 8])
def test_gradient_allreduce_equals_full_batch(tmp_path, world):
    _shard_backward(world, str(tmp_path))
    port = _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    rs = [torch.load(os.path.join(tmp_path, f'rank{r}.pt')) for r in range(world)]
    r0, r1 = rs[0], rs[1]
    G = _global_batch(world)
    for r in rs[1:]:
        assert torch.equal(r0['p'], r['p'])                       # broadcast made the replicas identical
        assert torch.equal(r0['g'], r['g'])                       # every rank holds the same reduced, clipped gradient
    assert [r['seed'] for r in rs] == [77 + i for i in range(world)]
    from ecg_representation_learning_amd.engine import ParamLayout
    from oracle import vit_oracle as O
    torch.manual_seed(1234)
    model = O.OracleEcgVit(config=Cfg(**CFG)).train()
    layout = ParamLayout([(n, tuple(p.shape)) for n, p in model.named_parameters()])
    p0 = torch.zeros(layout.total)
    for n, p in model.named_parameters():
        layout.view(p0, n).copy_(p.data)
    assert torch.equal(r0['p'], p0)                               # ... to rank 0's weights: those the shard gradients were taken on
    # GradExchange: the f32 forms equal the plain all-reduce bit for bit; bf16 on the wire stays within bf16 rounding of it
    # (world 2: a + b has one order; beyond that a ring's sum order depends on how the buffer is cut into buckets -> f32 rounding)
    for tag in ('f32_overlap', 'f32_single'):
        for r in rs:
            assert torch.equal(r['xchg'][tag], r0['xchg'][tag])
            if world == 2:
                assert torch.equal(r['xchg'][tag], r0['gavg'])
            else:
                assert float((r['xchg'][tag] - r0['gavg']).norm() / r0['gavg'].norm()) < 1e-6
    for tag in ('bf16_overlap', 'bf16_single'):
        for r in rs[1:]:
            assert torch.equal(r0['xchg'][tag], r['xchg'][tag])
        rel = float((r0['xchg'][tag] - r0['gavg']).norm() / r0['gavg'].norm())
        assert 0 < rel < BF16_WIRE_REL[world], (world, rel)
        worst = min(float(torch.nn.functional.cosine_similarity(layout.view(r0['xchg'][tag], n).flatten(), layout.view(r0['gavg'], n).flatten(), dim=0))
                    for n in layout.entries if float(layout.view(r0['gavg'], n).norm()) > 0)
        print(f'world {world} {tag}: reduced-gradient rel error {rel:.2e}, worst per-tensor cosine {worst:.6f}')
        assert worst >= 0.98, (world, tag, worst)
    # single-process full-batch reference
    x, y = O.synthetic_batch(G, length=400, seed=77)
    out = model(sample_values=x, labels=y)
    out.loss.backward()
    tn = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    g = torch.zeros(layout.total)
    for n, p in model.named_parameters():
        layout.view(g, n).copy_(p.grad)
    assert abs(float(r0['norm']) - float(tn)) / float(tn) < 1e-5
    assert float((r0['g'] - g).norm() / g.norm()) < 1e-5
    assert abs(float(out.loss.detach()) - sum(float(r['loss']) for r in rs) / world) < 1e-6   # mean of shard means


def _masked_named(mm):
    """(flat-layout name, parameter) of an OracleMaskedEcgVit in the package's order: the encoder's tensors, then the `pretrain.` extras"""
    own = [(n, p) for n, p in mm.encoder.named_parameters()]
    return own + [('pretrain.mask_token', mm.mask_token), ('pretrain.to_pixels.weight', mm.to_pixels.weight), ('pretrain.to_pixels.bias', mm.to_pixels.bias)]


def _worker_masked(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import ecg_representation_learning_amd as E
    from ecg_representation_learning_amd.engine import ParamLayout
    from oracle import vit_oracle as O
    torch.set_num_threads(2)
    cfg = Cfg(max_signal_length=400, patch_size=20, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64)
    torch.manual_seed(4321 + rank)
    mm = O.OracleMaskedEcgVit(O.OracleEcgVit(config=cfg)).train()
    named = _masked_named(mm)
    layout = ParamLayout([(n, tuple(p.shape)) for n, p in named])
    pflat = torch.zeros(layout.total)
    for n, p in named:
        layout.view(pflat, n).copy_(p.data)
        p.data = layout.view(pflat, n)
    E.ddp.broadcast_flat_(pflat, src=0)
    G, m = 8, 10
    x, _ = O.synthetic_batch(G, length=400, seed=77)
    idx = torch.stack([torch.randperm(20, generator=torch.Generator().manual_seed(100 + b))[:m] for b in range(G)]).to(torch.int32)   # the GLOBAL batch's masks
    lo, hi = E.ddp.shard_range(G, rank, world)
    out = mm(x[lo:hi], idx[lo:hi])
    out.loss.backward()
    gflat = torch.zeros(layout.total)
    for n, p in named:
        if p.grad is not None:      # cls_token and the classification head take no part in this objective: zero, as the HIP path writes them
            layout.view(gflat, n).copy_(p.grad)
    ranges = layout.buckets_in_ready_order(cfg.num_hidden_layers)
    outs = {}
    for tag, kw in (('overlap', dict(overlap=True)), ('single', dict(overlap=False))):
        g2 = gflat.clone()
        ex = E.ddp.GradExchange(ranges, **kw)
        ex.begin(g2)
        for name in ['head'] + [n for n, _ in ranges if n != 'head']:     # the masked backward's release order: head first (known at once)
            ex.bucket_ready(name)
        ex.finish()
        outs[tag] = g2 / ex.world
    torch.save(dict(p=pflat.clone(), loss=out.loss.detach(), g=outs, tags=[n for n, _ in ranges]), os.path.join(out_dir, f'mrank{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def test_masked_pretrain_gradient_exchange_equals_full_batch(tmp_path):
    """the data-parallel MASKED pre-train step (the north_star's DP loop is the pre-train step) on CPU, world 2, gloo: equal shards of records AND of
    their mask indices, the layout with the `pretrain.` extras behind the encoder (bucket order head, layers, embed, pretrain -- every element of
    the flat buffer in exactly one bucket), sum / world = the full-batch gradient of the mean-L1 loss"""
    world = 2
    port = _free_port()
    mp.spawn(_worker_masked, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f'mrank{r}.pt')) for r in range(world))
    assert torch.equal(r0['p'], r1['p']) and r0['tags'] == ['head', 'layer1', 'layer0', 'embed', 'pretrain']
    for tag in ('overlap', 'single'):
        assert torch.equal(r0['g'][tag], r1['g'][tag])
    assert torch.equal(r0['g']['overlap'], r0['g']['single'])
    from ecg_representation_learning_amd.engine import ParamLayout
    from oracle import vit_oracle as O
    cfg = Cfg(max_signal_length=400, patch_size=20, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64)
    torch.manual_seed(4321)
    mm = O.OracleMaskedEcgVit(O.OracleEcgVit(config=cfg)).train()
    named = _masked_named(mm)
    layout = ParamLayout([(n, tuple(p.shape)) for n, p in named])
    cover = sorted(v for _, v in layout.buckets_in_ready_order(2))
    assert cover[0][0] == 0 and cover[-1][1] == layout.total and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    x, _ = O.synthetic_batch(8, length=400, seed=77)
    idx = torch.stack([torch.randperm(20, generator=torch.Generator().manual_seed(100 + b))[:10] for b in range(8)]).to(torch.int32)
    out = mm(x, idx)
    out.loss.backward()
    g = torch.zeros(layout.total)
    for n, p in named:
        if p.grad is not None:
            layout.view(g, n).copy_(p.grad)
    assert float((r0['g']['overlap'] - g).norm() / g.norm()) < 1e-5
    assert abs(float(out.loss.detach()) - 0.5 * (float(r0['loss']) + float(r1['loss']))) < 1e-6
    for n in ('vit.mlp_head.0.weight', 'vit.mlp_head.1.weight', 'vit.cls_token'):
        assert float(layout.view(r0['g']['overlap'], n).abs().max()) == 0.0


def test_shard_range_contract():
    import ecg_representation_learning_amd as E
    assert [E.ddp.shard_range(4096, r, 8) for r in (0, 7)] == [(0, 512), (3584, 4096)]
    with pytest.raises(ValueError):
        E.ddp.shard_range(10, 0, 4)
    g = torch.ones(5)
    assert E.ddp.allreduce_flat_(g) == 1 and torch.equal(g, torch.ones(5))   # no process group: identity
