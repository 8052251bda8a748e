"""Iterative DP-SGD workload (the reference's APRIL-ANN example, SURVEY.md C22,
K13/K14, P4/P5): fused MFMA gradient kernel vs a PyTorch fp32 autograd
reference, the SGD kernel, the stopping rule, DP over ranks (gloo), and the
server/worker form through the coordinator.

APRIL-ANN itself is not available here, so parity with the reference's training
curve is unpinned; what is pinned is the math (autograd) and that the three
execution forms (1 rank, W ranks, server/worker jobs) agree."""
import contextlib
import io
import os
import socket
import threading

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import lua_mapreduce_1_amd as mr
from lua_mapreduce_1_amd.models import mlp_dpsgd as T
from lua_mapreduce_1_amd.ops import mlp as M
from lua_mapreduce_1_amd.runtime import coordinator
from lua_mapreduce_1_amd.utils import digits

DATA = digits.synthetic(seed=3)


def _data_t(device):
    tx, ty, vx, vy = DATA
    return torch.from_numpy(tx).to(device), torch.from_numpy(ty).to(device)


def test_layout_and_init():
    L = M.LAYOUT
    assert L.size == 256 * 128 + 128 + 128 * 10 + 10
    w = M.init_params(1)
    assert w.shape == (L.size,)
    assert float(w[L.w1].abs().max()) <= 1 / 16 + 1e-6
    assert torch.equal(w, M.init_params(1))


def test_cpu_grad_matches_finite_differences():
    X, y = _data_t("cpu")
    idx = torch.arange(8, dtype=torch.int32)
    w = M.init_params(5).double()
    Xd = X.double()
    g, _ = M.reference_forward_backward(Xd, y, idx, w)
    for p in (3, M.LAYOUT.b1.start + 2, M.LAYOUT.w2.start + 7, M.LAYOUT.b2.start + 1):
        e = torch.zeros_like(w)
        e[p] = 1e-6
        _, lp = M.reference_forward_backward(Xd, y, idx, w + e, want_grad=False)
        _, lm = M.reference_forward_backward(Xd, y, idx, w - e, want_grad=False)
        fd = (lp[0] - lm[0]) / 2e-6
        assert abs(float(fd) - float(g[p])) < 1e-5 * max(1.0, abs(float(fd)))


def test_sgd_cpu_semantics():
    L = M.LAYOUT
    w = torch.ones(L.size)
    g = torch.full((L.size,), 2.0)
    v = torch.zeros(L.size)
    M.sgd_step(w, g, v, lr=0.1, momentum=0.5, weight_decay=0.01, scale=0.5)
    assert torch.allclose(w[L.w1], torch.full_like(w[L.w1], 1 - 0.1 * (1.0 + 0.01)))
    assert torch.allclose(w[L.b2], torch.full_like(w[L.b2], 1 - 0.1 * 1.0))


def test_stop_rule():
    s = T.StopRule(min_epochs=3, max_epochs=10)
    vals = [5, 4, 3, 3.5, 3.6, 3.7, 3.8]
    go = [s.update(1.0, v) for v in vals]
    # best at epoch 3 -> stop once epoch >= 6
    assert go == [True, True, True, True, True, False, False]
    s = T.StopRule(min_epochs=1, max_epochs=4)
    assert [s.update(1.0, 10 - i) for i in range(4)] == [True, True, True, False]


def test_train_spmd_cpu_learns():
    r = T.train_spmd("cpu", data=DATA, epochs=12)
    h = r["history"]
    assert h[-1]["va_loss"] < h[0]["va_loss"] - 0.1
    assert len(h) == 12


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from lua_mapreduce_1_amd.parallel import dist as D
    D.init_from_env(backend="gloo", use_gpu=False)
    r = T.train_spmd("cpu", data=DATA, epochs=5)
    if rank == 0:
        q.put(r["params"].numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_dp_over_ranks_matches_single_rank(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    w_dp = q.get(timeout=240)  # before join: a child cannot exit with unflushed queue data
    for p in procs:
        p.join(240)
    assert all(p.exitcode == 0 for p in procs)
    w_1 = T.train_spmd("cpu", data=DATA, epochs=5)["params"].numpy()
    np.testing.assert_allclose(w_dp, w_1, rtol=1e-4, atol=1e-5)


def test_server_worker_digits_mlp_matches_spmd():
    """The map/reduce/final form (4 jobs of one bunch, reduce per weight name,
    finalfn optimizer step, "loop") reproduces the SPMD trainer."""
    from lua_mapreduce_1_amd.examples import DigitsMLP as ex
    cs = coordinator.start_local()
    mod = "lua_mapreduce_1_amd.examples.DigitsMLP"
    ex._data_cache["synthetic"] = DATA
    ex._trainer = None
    s = mr.server.new(cs, "mr_exp_digits")
    s.poll_sleep = 0.02
    s.quiet = True
    s.configure(dict(taskfn=mod, mapfn=mod, partitionfn=mod, reducefn=mod, finalfn=mod, storage="gridfs",
                     init_args=[cs, "synthetic", 4]))
    w = mr.worker.new(cs, "mr_exp_digits")
    w.configure(verbose=False, poll_sleep=0.02, max_iter=5)
    t = threading.Thread(target=w.execute, daemon=True)
    t.start()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        s.loop()
    lines = [ln for ln in buf.getvalue().splitlines() if ln.strip()]
    assert len(lines) == 4
    conf = mr.persistent_table("conf", cs, ex.DB)
    assert conf.finished and conf.epoch == 4
    r = T.train_spmd("cpu", data=DATA, epochs=4)
    hist = [h["va_loss"] for h in r["history"]]
    np.testing.assert_allclose([h[2] for h in conf.history], hist, rtol=1e-4)


# ---------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("B", [128, 512, 37, 16, 1])
def test_fused_grad_kernel_matches_fp32_reference(gpu, B):
    X, y = _data_t(gpu)
    g = torch.Generator().manual_seed(B)
    idx = torch.randint(0, X.shape[0], (B,), generator=g, dtype=torch.int32)
    w = M.init_params(11)
    ref_g, ref_l = M.reference_forward_backward(X.cpu(), y.cpu(), idx, w)
    grads = torch.empty(M.LAYOUT.size, device=gpu)
    loss = M.grad_step(X, y, idx.to(gpu), w.to(gpu), grads)
    torch.cuda.synchronize()
    gd = grads.cpu()
    scale = ref_g.abs().max()
    assert torch.allclose(gd, ref_g, rtol=1e-4, atol=1e-5 * float(scale) + 1e-6), float((gd - ref_g).abs().max())
    assert torch.allclose(loss.cpu(), ref_l, rtol=1e-5, atol=1e-4)


@pytest.mark.gpu
def test_fused_kernel_repeatable_and_forward_only(gpu):
    X, y = _data_t(gpu)
    idx = torch.arange(200, dtype=torch.int32, device=gpu)
    w = M.init_params(2).to(gpu)
    ws = M.GradWorkspace(512, gpu)
    g1 = torch.empty(M.LAYOUT.size, device=gpu)
    g2 = torch.empty_like(g1)
    l1 = M.grad_step(X, y, idx, w, g1, ws).clone()
    M.grad_step(X, y, idx, w, g2, ws)
    assert torch.equal(g1, g2)  # deterministic block-ordered reduction
    lf = M.grad_step(X, y, idx, w, None, ws, want_grad=False)
    assert torch.allclose(lf, l1)
    assert int(ws.counter.item()) == 0


@pytest.mark.gpu
def test_sgd_kernel_matches_cpu(gpu):
    n = M.LAYOUT.size
    g = torch.Generator().manual_seed(0)
    w, gr, v = (torch.randn(n, generator=g) for _ in range(3))
    wd, grd, vd = w.to(gpu), gr.to(gpu), v.to(gpu)
    M.sgd_step(w, gr, v, 0.01, 0.02, 1e-4, 0.3)
    M.sgd_step(wd, grd, vd, 0.01, 0.02, 1e-4, 0.3)
    assert torch.allclose(wd.cpu(), w, atol=1e-6) and torch.allclose(vd.cpu(), v, atol=1e-6)


def _resume_check(device, ckpt, graphs=None):
    full = T.train_spmd(device, data=DATA, epochs=8, graphs=graphs)
    first = T.train_spmd(device, data=DATA, epochs=5, graphs=graphs, checkpoint=ckpt)
    assert first["resumed_from"] == 0
    rest = T.train_spmd(device, data=DATA, epochs=8, graphs=graphs, checkpoint=ckpt)
    assert rest["resumed_from"] == 5
    assert torch.equal(rest["params"], full["params"])
    assert [h["va_loss"] for h in rest["history"]] == [h["va_loss"] for h in full["history"]]


def test_checkpoint_resume_is_bit_identical(tmp_path):
    """A run stopped after epoch 5 and relaunched from its snapshot ends with
    the parameters of an uninterrupted 8-epoch run (APRIL-ANN restore,
    common.lua:57-77); a finished run's snapshot is not resumed."""
    ckpt = str(tmp_path / "mlp.pt")
    _resume_check("cpu", ckpt)
    T.train_spmd("cpu", data=DATA, hyper={"min_epochs": 2, "max_epochs": 3}, checkpoint=ckpt)
    assert T.load_checkpoint(ckpt) is None  # finished by the stopping rule
    assert T.train_spmd("cpu", data=DATA, epochs=2, checkpoint=ckpt)["resumed_from"] == 0


@pytest.mark.gpu
def test_checkpoint_resume_graphs_gpu(gpu, tmp_path):
    _resume_check(gpu, str(tmp_path / "mlp.pt"), graphs=True)


@pytest.mark.gpu
def test_train_spmd_gpu_matches_cpu(gpu):
    rg = T.train_spmd(gpu, data=DATA, epochs=6)
    rc = T.train_spmd("cpu", data=DATA, epochs=6)
    np.testing.assert_allclose([h["va_loss"] for h in rg["history"]], [h["va_loss"] for h in rc["history"]],
                               rtol=1e-4)


@pytest.mark.gpu
def test_graph_epochs_equal_eager(gpu):
    rg = T.train_spmd(gpu, data=DATA, epochs=5, graphs=True)
    re_ = T.train_spmd(gpu, data=DATA, epochs=5, graphs=False)
    assert torch.equal(rg["params"], re_["params"])
    assert [h["va_loss"] for h in rg["history"]] == [h["va_loss"] for h in re_["history"]]


# a copy of the reference's misc/digits.png
REF_PNG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "digits.png")


def test_reference_digits_png_trains():
    """The reference's own dataset (misc/digits.png: 100 rows x 10 glyphs of
    16x16, read as pixels only), the APRIL-ANN schedule until the stopping rule
    (min 20 / max 40 epochs): validation loss and accuracy must improve well
    beyond chance — parity with the reference's training curve is unpinned (no
    Lua/APRIL-ANN here to produce one)."""
    data = digits.load(REF_PNG)
    assert data[0].shape == (800, 256) and data[2].shape == (200, 256)
    assert 0.0 <= float(data[0].min()) and float(data[0].max()) <= 1.0
    r = T.train_spmd("cpu", data=data)
    h = r["history"]
    assert 20 <= len(h) <= 40
    assert h[-1]["va_loss"] < h[0]["va_loss"] - 0.5
    assert h[-1]["va_acc"] > 0.8  # 0.91 after 40 epochs here
