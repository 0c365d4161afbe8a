"""GPU: the N > 1 step on ONE GPU.  Two ranks (gloo; RCCL refuses two ranks per device) run FinetuneStep / PretrainStep under
hipGraph replay with the bucketed gradient all-reduce between the backward phases (collectives on the side stream, 1/world
folded into AdamW).  Requirements: parameters bit-identical across ranks, and equal (fp32 mode) to ONE process stepping the
2B-image global batch.  Reference: DDP wrap FSC_finetune_cross.py:178-183,230; util/misc.py:225-257."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_retry(make_cmd, env, attempts=2):
    """Multi-process launches rendezvous over a fresh local port; a transient start-up failure of the process group (seen once in
    ~30 runs on the GPU pool: RCCL communicator set-up) gets one more attempt on another port before the test fails."""
    r = None
    for k in range(attempts):
        try:     # (a start-up that hangs -- seen once on the pool, in the RCCL one-rank bench -- counts as a failed attempt, not as 15 idle minutes)
            r = subprocess.run(make_cmd(), cwd=ROOT, capture_output=True, text=True, timeout=420, env=env)
        except subprocess.TimeoutExpired as e:
            if k + 1 == attempts:
                raise
            print("attempt %d timed out: %s" % (k, (e.stderr or b"")[-1500:]))
            continue
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def launch(what, outdir, nproc=2, backend="gloo", extra_env=None):
    cmd = lambda: [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
                   "--master-port", str(free_port()), os.path.join(ROOT, "tests", "ddp_gpu_worker.py"), what, str(outdir), backend]
    run_retry(cmd, dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {})))
    return [torch.load(os.path.join(outdir, "%s_rank%d.pt" % (what, k)), weights_only=False) for k in range(nproc)]


@pytest.mark.parametrize("what", ["finetune", "pretrain"])
def test_two_ranks_on_one_gpu_match_single_process(what, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ddp_gpu_worker as Wk
    r0, r1 = launch(what, tmp_path)
    for k in r0["params"]:
        assert torch.equal(r0["params"][k], r1["params"][k]), k            # ranks stay bit-identical
    single, losses = (Wk.run_finetune if what == "finetune" else Wk.run_pretrain)(0, 1, 4)
    # the logged loss of a rank is the loss of ITS half; their mean is the global-batch loss
    for a, b, c in zip(r0["losses"], r1["losses"], losses):
        assert abs(0.5 * (a + b) - c) <= 2e-4 * abs(c), (a, b, c)
    lr = 1e-3
    n_steps = len(losses)
    for k, p in single.named_parameters():
        d = (p.detach().cpu().double() - r0["params"][k].double()).abs()
        # same tolerance logic as test_trainer_gpu: AdamW steps are ~lr per element; summation order differs (2 x B=2 vs B=4)
        assert d.pow(2).mean().sqrt().item() <= 0.03 * lr * n_steps, (k, d.pow(2).mean().sqrt().item())
        if not k.startswith("decoder_proj"):
            assert d.max().item() <= 0.3 * lr * n_steps, (k, d.max().item())


def test_per_rank_shot_num_matches_oracle_mean_gradient(tmp_path):
    """Reference semantics of the only multi-GPU path: every rank draws its own shot_num (FSC_finetune_cross.py:276-284) and DDP with
    find_unused_parameters=True (:230) averages whatever gradients exist -- a parameter set unused on one rank contributes zeros, one
    unused on EVERY rank keeps grad None and is skipped by AdamW.  Two ranks (gloo, one GPU, graph replay) with the schedule
    rank 0: [3, 0, 1, 0], rank 1: [0, 0, 3, 2] against the oracle: gradients of each half-batch under its own shot_num, averaged, fed
    to the real torch.optim.AdamW.  Iteration 0: rank 0 has no shot_token gradient, rank 1 none for the exemplar CNN -- both sets are
    reduced (zero-filled where absent) and stepped; iteration 1: the exemplar CNN is stepped with a zero gradient (torch 1.13
    zero_grad leaves zeros); the last iteration's counts are all-gathered instead of passed in."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ddp_gpu_worker as Wk
    from test_trainer_gpu import TorchAdamW
    from oracle import countr_ref as R, weights as W
    r0, r1 = launch("finetune_prs", tmp_path)
    for k in r0["params"]:
        assert torch.equal(r0["params"][k], r1["params"][k]), k            # ranks stay bit-identical
    assert r0["group_steps"] == [4, 4, 4] and r1["group_steps"] == [4, 4, 4]
    lr, name = 1e-3, "tiny_test"
    sd = W.make_state_dict(name, seed=3)
    ref = TorchAdamW(sd, lr, 1e-4)
    for it, shots in enumerate(Wk.PRS):
        imgs, boxes, gt, mask = W.make_inputs(batch=4, shots=3, seed=140 + it)
        cur = ref.state_dict_f32(sd)
        for r, S in enumerate(shots):
            sl = slice(2 * r, 2 * r + 2)
            _out, rloss, rg = R.loss_and_grads(cur, imgs[sl], boxes[sl], gt[sl], mask, S, name)
            got = (r0, r1)[r]["losses"][it]
            assert abs(got - rloss.item()) <= 2e-3 * abs(rloss.item()), (it, r, S, got, rloss.item())
            ref.accumulate(rg, scale=0.5)
        ref.step()
    n = len(Wk.PRS)
    for k, v in ref.p.items():
        d = (r0["params"][k].double() - v.detach()).abs()
        assert d.pow(2).mean().sqrt().item() <= 0.03 * lr * n, (k, d.pow(2).mean().sqrt().item())
        if not k.startswith("decoder_proj"):
            assert d.max().item() <= 0.25 * lr * n, (k, d.max().item())
    # shot_token and the exemplar CNN both moved in iteration 0 although each was unused on one rank
    assert not np.array_equal(r0["params"]["shot_token"].numpy(), sd["shot_token"])


def test_two_ranks_at_the_real_config(tmp_path):
    """The same two-rank step at BASELINE config 3's per-GPU shape -- ViT-B/16, bf16, 8 images per rank, graph replay (the tiny fp32
    model above proves the arithmetic, this one the production plans: lean GEMM kernels, fused attention backward, 4 buckets of
    11.8 / 35 / 6.2 MB / 2 KB reduced between the replayed phases).  Ranks must stay bit-identical over six steps with every shot
    count, and their mean loss must follow ONE process stepping the 16-image batch (bf16: same data, other summation order)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ddp_gpu_worker as Wk
    r0, r1 = launch("finetune_real", tmp_path)
    assert len(r0["params"]) > 50
    for k in r0["params"]:
        assert torch.equal(r0["params"][k], r1["params"][k]), k
    assert all(torch.isfinite(torch.tensor(r0["losses"] + r1["losses"])))
    single, losses = Wk.run_finetune_real(0, 1, per_rank=16)
    for a, b, c in zip(r0["losses"], r1["losses"], losses):
        assert abs(0.5 * (a + b) - c) <= 2e-2 * abs(c), (a, b, c)
    lr, n_steps = 1e-4, len(losses)
    worst = 0.0
    for k, p in single.named_parameters():
        if k in r0["params"]:
            d = (p.detach().cpu().double() - r0["params"][k].double())
            worst = max(worst, d.pow(2).mean().sqrt().item())
    # AdamW moves ~lr per element and step whatever the gradient's size, so bf16 noise on near-zero gradient elements flips whole steps:
    # the bound only says "the same trajectory" (measured 0.4 lr n); the arithmetic of the exchange is pinned by the fp32 test above
    assert worst <= 0.6 * lr * n_steps, worst


@pytest.mark.parametrize("what", ["finetune", "pretrain"])
def test_bucket_gradients_are_final_when_their_all_reduce_starts(what):
    """The overlap relies on ONE ordering fact: when phase i has run, no later phase writes or accumulates into the gradient range of
    bucket i (its all-reduce starts right there on the side stream and would race with such a write).  Proof by poison: after each
    phase the finished bucket is snapshotted and the SAME range is then filled with NaN in eng.G; the remaining phases run; the range
    must still be all-NaN bit patterns written by us (nothing overwrote it) and -- run again without poison -- equal the snapshot bit
    for bit (nothing accumulated into it).  Finetune: buckets head | decoder blocks | exemplar CNN / shot_token; pretrain: decoder
    side + six encoder groups."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ddp_gpu_worker as Wk
    from countr_amd.trainer import FinetuneStep, PretrainStep
    import numpy as np
    from oracle import weights as W
    if what == "finetune":
        m = Wk.finetune_model("bf16")
        step = FinetuneStep(m, batch=2, lr=1e-3, use_graph=False)
        imgs, boxes, gt, mask = W.make_inputs(batch=2, shots=3, seed=7)
        keys = [3, 0]
        load = lambda S: step.load(*(torch.from_numpy(a).cuda() for a in (imgs, boxes, gt, mask)), S)
    else:
        m = Wk.pretrain_model("bf16")
        step = PretrainStep(m, batch=2, mask_ratio=0.5, lr=1e-3, use_graph=False)
        rs = np.random.RandomState(3)
        img = torch.from_numpy(rs.uniform(0, 1, size=(2, 3, 384, 384)).astype(np.float32)).cuda()
        ids = torch.from_numpy(np.stack([rs.permutation(m.patch_embed.num_patches) for _ in range(2)])).cuda()
        keys = [step.K]
        load = lambda S: step.load(img, ids_shuffle=ids)
    eng = step.eng
    for key in keys:
        snaps = None
        for poison in (False, True):
            load(key)
            eng.G.zero_()
            phases = step._phases(key)
            buckets = step.sync.buckets
            got = {}
            with torch.cuda.stream(step.stream):
                for i, (name, fn, gkey) in enumerate(phases):
                    fn(gkey)
                    done = [i] if i + 1 < len(phases) else list(range(i, len(buckets)))    # the last phase finishes all remaining buckets
                    for b in done:
                        s0, e0 = buckets[b]
                        got[b] = eng.G[s0:e0].clone()
                        if poison:
                            eng.G[s0:e0] = float("nan")
            torch.cuda.synchronize()
            if not poison:
                snaps = {b: v for b, v in got.items()}
                final = eng.G.clone()
                for b, (s0, e0) in enumerate(buckets):
                    assert torch.equal(final[s0:e0], snaps[b]), (what, key, b)          # nothing accumulated into a finished bucket
            else:
                for b, (s0, e0) in enumerate(buckets):
                    assert torch.isnan(eng.G[s0:e0]).all(), (what, key, b)               # nothing overwrote a poisoned (finished) bucket
                for b in got:
                    assert torch.equal(got[b], snaps[b]), (what, key, b)                 # and the poison did not leak into later buckets


def test_bench_self_launch_two_ranks():
    """`python bench.py --gpus 2` started like the N = 1 run (no torch.distributed.run) re-launches itself with one rank per
    requested GPU and reports n_gpus = 2 (gloo on the single GPU of this box)."""
    import json
    r = run_retry(lambda: [sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo", "--steps", "3", "--warmup", "2", "--no-cpu-baseline",
                           "--full"], dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 16 and j["value"] > 0
    # the timed step object is checked against the oracle outside the timed regions -- at N > 1 the all-reduced flat gradient against
    # the SUM of the oracle's per-rank gradients (what the collective carried)
    assert j["parity_checked"] is True and j["parity"]["gradient_tensors"] >= 55 and "sum of the oracle" in j["parity"]["gradients"]
    assert j["parity"]["min_cos"] > 0.999 and j["parity"]["loss_rel_err"] < 1e-2


@pytest.mark.parametrize("what", ["finetune", "pretrain"])
def test_rccl_path_with_one_rank(what, tmp_path):
    """The REAL RCCL path on the single GPU: backend "nccl" (= RCCL), a one-rank group, COUNTR_FORCE_COMM=1 so that GradSync issues
    every bucket all-reduce (communicator set-up, collectives on the side stream between the graph replays, joins) although the
    sum over one rank is the identity.  Result must be bit-identical to the same step without any communication."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ddp_gpu_worker as Wk
    (r0,) = launch(what, tmp_path, nproc=1, backend="nccl", extra_env={"COUNTR_FORCE_COMM": "1"})
    single, losses = (Wk.run_finetune if what == "finetune" else Wk.run_pretrain)(0, 1, 4)
    assert r0["losses"] == losses
    for k, p in single.named_parameters():
        assert torch.equal(p.detach().cpu(), r0["params"][k]), k
    # over RCCL the collectives are CAPTURED: the communicating step is one graph ("allc"), not one graph per phase
    assert r0["graph_kinds"] == ["allc"], r0["graph_kinds"]
    # ... and with COUNTR_GRAPH_COMM=0 (host-issued collectives between per-phase graphs, what gloo always does) the result is the same
    (r1,) = launch(what, tmp_path, nproc=1, backend="nccl", extra_env={"COUNTR_FORCE_COMM": "1", "COUNTR_GRAPH_COMM": "0"})
    assert r1["losses"] == losses and "allc" not in r1["graph_kinds"] and len(r1["graph_kinds"]) >= 3
    for k, p in single.named_parameters():
        assert torch.equal(p.detach().cpu(), r1["params"][k]), k


def test_bench_rccl_one_rank():
    """bench.py --full through torch.distributed.run with backend nccl on one rank and forced collectives: the launch line the driver uses
    for N > 1, exercised as far as one GPU allows."""
    import json
    cmd = lambda: [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                   "--master-port", str(free_port()), "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--no-cpu-baseline", "--full"]
    r = run_retry(cmd, dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", COUNTR_FORCE_COMM="1", COUNTR_BENCH_INIT_PG="1"))
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 1 and j["value"] > 0 and j["parity_checked"] is True
    # captured collectives: one graph per step -- with the NEXT batch's frozen-encoder forward on its own lane of it (round 6; the
    # optimizer update then runs at the tail of its step, beside that lane; COUNTR_PIPELINE_ENCODER=0: the deferred update of round 5)
    assert j["config"]["encoder_pipelining"].startswith("on") and j["config"]["optimizer_update"] == "at the tail of its step"
    r = run_retry(cmd, dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", COUNTR_FORCE_COMM="1", COUNTR_BENCH_INIT_PG="1", COUNTR_PIPELINE_ENCODER="0"))
    j0 = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j0["config"]["encoder_pipelining"] == "off" and j0["config"]["optimizer_update"].startswith("deferred") and j0["parity_checked"] is True
    assert j["multi_gpu_safe_mode"]["ms_per_step_host_issued_first"] > 0  # the host-issued form was measured first (the watchdog's line)


def test_bench_watchdog_prints_the_host_issued_line_when_captured_collectives_hang():
    """A hang in the captured-collective form cannot be caught as an exception: bench.py keeps the line it measured in the host-issued form
    first and a watchdog prints it when nothing moves for COUNTR_BENCH_WATCHDOG_S seconds (COUNTR_BENCH_FAKE_HANG=1 puts the main thread
    to sleep behind the capture); every rank leaves with exit code 0, so the driver's scaling run still gets a valid line."""
    import json
    cmd = lambda: [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                   "--master-port", str(free_port()), "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--no-cpu-baseline"]
    r = run_retry(cmd, dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", COUNTR_FORCE_COMM="1", COUNTR_BENCH_INIT_PG="1",
                            COUNTR_BENCH_FAKE_HANG="1", COUNTR_BENCH_WATCHDOG_S="5"))
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 1 and j["value"] > 0 and j["steps"] == 3 and j["parity_checked"] is False
    assert "made no progress for 5 s" in j["multi_gpu"]["fallback"] and "issued by the host" in j["multi_gpu"]["collectives"]


@pytest.mark.parametrize("warmup", [3, 5, 8])
def test_bench_parity_guard_holds_behind_any_warmup(warmup):
    """bench.py's own parity check runs behind the caller's warm-up steps, on a torch-initialised model whose count swings through zero
    while the first steps move the last bias (-30 after three steps, +530 after five): relative to the count itself a 2-count bf16 error
    read 9.7 % after --warmup 3 and failed the run; 54 instead of 58 tensors carried a judgeable gradient after --warmup 8.  The guard
    measures counts against the density map's mass and accepts >= 40 tensors.  --warmup 5 --steps 20 is the driver's command."""
    import json
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20" if warmup == 5 else "3", "--warmup", str(warmup), "--reps", "1",
                        "--full", "--no-other", "--no-cpu-baseline", "--no-families", "--no-b32"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["parity_checked"] is True and j["parity"]["count_rel_err"] < 5e-2 and j["parity"]["gradient_tensors"] >= 40
