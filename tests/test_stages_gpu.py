"""Stage audit of the 16-bit engines' exemplar CNN (decoder_proj1..4: conv, InstanceNorm, ReLU, pool) and density head
(decode_head0..3: conv, GroupNorm, ReLU, bilinear x2), launch by launch.

The whole-model tests compare these places with the fp32 oracle, whose bars (cos > 0.97 / 0.999) cannot be tightened: bf16 rounding
through InstanceNorm amplifies legitimately.  Here the reference changes instead of the bar: a train step runs the normal way, then the
SAME launch lists (Engine.plan(B, S, True).fwd / bwd_head / bwd_rest / bwd_tok) run one launch at a time, and every stage is compared
with fp64 arithmetic on THAT LAUNCH'S OWN INPUTS -- the rounded buffers the engine left in place (tests/stagecheck.py).  Every stage is
then one rounding of an fp32 computation: 16-bit outputs meet tests/halfprec.py's element-wise bound with the fp32 bar (2e-4) as floor,
fp32 outputs and parameter gradients 2e-4 of the largest value, statistics 3e-6.  Nothing is excluded except, in a GroupNorm backward,
the elements whose fp64 pre-activation lies within 2^-16 (|gamma xhat| + |beta|) of zero (the kernel decides the ReLU gate from an fp32
y); the stage asserts on the reference alone that these are at most 1e-4 of the map (the CPU oracle counts 0 to 3.4e-6 of the four
head maps for the two inputs used here).

Plans: (B, S) = (2, 3) -- two images show a wrong per-image stride, 6 crops give the first convolution's weight gradient 48-pixel
ranges -- and (1, 1): one crop is a 64-pixel map for decoder_proj4, fewer k-tiles than split-K slabs."""
import collections

import pytest
import torch

import halfprec as HP
import stagecheck as SC
from oracle import countr_ref as R
from oracle import weights as W

pytestmark = pytest.mark.gpu
MODEL = "mae_vit_base_patch16"


def build(precision, seed=0, model=MODEL):
    """As tests/test_model_gpu.py builds it."""
    import models_mae_cross as mm
    m = mm.__dict__[model](norm_pix_loss=False, precision=precision)
    sd = W.make_state_dict(model, seed=seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.to("cuda")
    m.eval()
    return m, sd


PLANS = [(2, 3, 1), (1, 1, 2)]          # (B, S, make_inputs seed)
PLAN_IDS = ["b2_s3", "b1_s1"]
PROJ_C = [3, 64, 128, 256, 512]
Trace = collections.namedtuple("Trace", "fl B S eng buf snap grads gemms mismatched what")


@pytest.fixture(scope="module")
def models():
    """flavour -> the model in that precision, built once per module."""
    built = {}

    def get(fl):
        if fl not in built:
            built[fl] = build("bf16" if fl is HP.BF16 else "fp16")[0]
        return built[fl]
    return get


# what the audit reads, all of it written in full by some launch: overwritten with a marker value between the normal and the stepped run,
# so that a launch the stepped run left out cannot hide behind what the normal run put there (ytok keeps its zero padding rows)
AUDITED = (["c%d" % i for i in (1, 2, 3, 4)] + ["ch%d" % i for i in (1, 2, 3, 4)] + ["p%d" % i for i in (1, 2, 3)] +
           ["instats%d" % i for i in (1, 2, 3, 4)] + ["dc%d" % i for i in (1, 2, 3, 4)] + ["dp%d" % i for i in (1, 2, 3)] +
           ["dy_tok", "dyt", "dn", "o1", "out", "d1", "ddn"] + ["hc%d" % i for i in range(4)] + ["hstats%d" % i for i in range(4)] +
           ["hu%d" % i for i in range(3)])
SCRATCH = ["hact_tmp", "dpre", "dup", "dact"]
MARKER = 777.0


def _gemm_record(op):
    a = op[2]
    return dict(modeA=int(op[1][2]), modeB=int(op[1][3]), M=a.M, N=a.N, K=a.K, splitk=a.splitk, A=a.A, B=a.B, C=a.C, partial=a.partial)


def _audit(fl, m, B, S, seed):
    """One train step the normal way (module forward, loss, backward), then the same launches one at a time with the shared scratch
    maps cloned behind the launch that writes them."""
    eng = m._engine()
    imgs, boxes, gt, mask = [torch.from_numpy(a).cuda() for a in W.make_inputs(batch=B, shots=3, seed=seed)]
    for q in m.parameters():
        q.grad = None
    m.train()
    out = m(imgs, boxes, S)
    R.masked_mse_loss(out, gt, mask).backward()
    m.eval()
    torch.cuda.synchronize()
    out0 = out.detach().clone()
    grads0 = {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}
    p = eng.plan(B, S, True)
    ws, snap, gemms, order = eng._ws, {}, [], {"gn_fwd": 0, "gn_bwd": 3}
    for t_ in [p.buf[k] for k in AUDITED] + [ws[k] for k in SCRATCH] + [p.buf["ytok"][:B * S], eng.G]:
        t_.fill_(MARKER)

    def behind(op):
        name, a = op[0].__name__, op[1]
        if name == "countr_gemm":
            gemms.append(_gemm_record(op))
        elif name in ("countr_groupnorm_relu_fwd", "countr_groupnorm_relu_fwd_rows"):
            k = 0 if name == "countr_groupnorm_relu_fwd" else 1       # (x, [rows,] gamma, beta, y, w1, b1, out1, stats, ws, B, HW, ...)
            if a[3 + k] is not None:
                assert a[3 + k] == ws["hact_tmp"].data_ptr()
                snap["hact%d" % order["gn_fwd"]] = ws["hact_tmp"][:a[9 + k] * a[10 + k] * 256].clone()
            order["gn_fwd"] += 1
        elif name == "countr_groupnorm_relu_bwd":      # (x, dy, d1, w1, stats, gamma, beta, dx, dgamma, dbeta, dw1, db1, ws, B, HW, ...)
            assert a[7] == ws["dpre"].data_ptr()
            snap["dpre%d" % order["gn_bwd"]] = ws["dpre"][:a[13] * a[14] * 256].clone()
            order["gn_bwd"] -= 1
        elif name == "countr_upsample2x_bwd" and a[5] == 256:       # (dout, din, B, H, W, C, dtype): dup of layer i + 1 -> dact of layer i
            assert a[0] == ws["dup"].data_ptr() and a[1] == ws["dact"].data_ptr()
            i = order["gn_bwd"]
            snap["dup%d" % (i + 1)] = ws["dup"][:a[2] * 4 * a[3] * a[4] * 256].clone()
            snap["dact%d" % i] = ws["dact"][:a[2] * a[3] * a[4] * 256].clone()

    def stepped(ops):
        for op in ops:
            if op[0] is None:          # a schedule marker
                continue
            eng.run([op])
            torch.cuda.synchronize()
            behind(op)

    stepped(p.fwd)
    snap["ytok_fwd"] = p.buf["ytok"].clone()
    for ops in (p.bwd_head, p.bwd_rest, p.bwd_tok):
        stepped(ops)
    grads = {k: eng.gview(k).clone() for k in grads0}
    mismatched = [] if torch.equal(p.buf["out"], out0) else ["out"]
    mismatched += [k for k in grads0 if not torch.equal(grads[k], grads0[k])]
    return Trace(fl, B, S, eng, p.buf, snap, grads, gemms, mismatched, "%s B%d S%d: " % (HP.FLAVOUR_IDS[HP.FLAVOURS.index(fl)], B, S))


@pytest.fixture(scope="module", params=[(fl, plan) for fl in HP.FLAVOURS for plan in PLANS],
                ids=["%s-%s" % (f, q) for f in HP.FLAVOUR_IDS for q in PLAN_IDS])
def tr(request, models):
    fl, plan = request.param
    return _audit(fl, models(fl), *plan)


def gemm(t, **match):
    """(modeA, modeB, M, N, K, splitk) of the recorded countr_gemm launch with these argument values, for a failure message."""
    for g in t.gemms:
        if all(g[k] == v for k, v in match.items()):
            return " gemm (modeA, modeB, M, N, K, splitk) = (%d, %d, %d, %d, %d, %d)" % (g["modeA"], g["modeB"], g["M"], g["N"], g["K"], g["splitk"])
    return " (no recorded gemm matches %s)" % sorted(match)


def proj_maps(t):
    """The exemplar CNN's inputs per layer as NHWC maps: boxes, p1..3."""
    return [t.buf["boxes"].permute(0, 2, 3, 1)] + [t.buf["p%d" % i] for i in (1, 2, 3)]


def test_stepped_run_is_bit_identical_to_the_normal_run(tr):
    """The audit looked at the computation production runs, the side-lane schedule of fwd_par included: the density map and every
    parameter gradient of the launch-by-launch run equal the module's, bit for bit."""
    assert tr.grads and not tr.mismatched, (tr.what, tr.mismatched)
    assert all(("hact%d" % i) in tr.snap for i in range(3)) and all(("dpre%d" % i) in tr.snap for i in range(4))
    assert all(("dup%d" % (i + 1)) in tr.snap and ("dact%d" % i) in tr.snap for i in range(3))


def test_weight_shadows_are_the_rounded_permutations_of_the_masters(tr):
    """What the stage references multiply with: Wf is the master rounded once in OHWI order, Wd the same values in dgrad form."""
    eng = tr.eng
    for n in eng.conv_names:
        w = eng.pview(n)
        wf = eng.Wf[n].view(w.shape[0], 3, 3, w.shape[1])
        assert torch.equal(wf, SC.ohwi(w).to(tr.fl.dtype)), (tr.what, n, "Wf")
        assert torch.equal(SC.ohwi_of_dgrad_form(eng.Wd[n], w.shape[0], w.shape[1]), wf), (tr.what, n, "Wd")


def test_exemplar_cnn_forward_stages(tr):
    t, buf, eng, fl = tr, tr.buf, tr.eng, tr.fl
    BS, maps = t.B * t.S, proj_maps(tr)
    for i in (1, 2, 3, 4):
        what = "%sdecoder_proj%d " % (t.what, i)
        wn, c, ch = "decoder_proj%d.0.weight" % i, buf["c%d" % i], buf["ch%d" % i]
        H = c.shape[1]
        if i == 1:
            ref, which = SC.conv3x3(maps[0], SC.ohwi(eng.pview(wn)), eng.pview(wn[:-6] + "bias")), " countr_conv3x3_c3_fwd"
        else:
            ref = SC.conv3x3(maps[i - 1], eng.Wf[wn].view(PROJ_C[i], 3, 3, PROJ_C[i - 1]), eng.pview(wn[:-6] + "bias"))
            which = gemm(t, A=maps[i - 1].data_ptr(), K=9 * PROJ_C[i - 1])
        SC.assert_f32(c, ref, what + "conv output c%d" % i + which)
        stats = SC.instnorm_stats(c)
        SC.assert_stats(buf["instats%d" % i], stats, what + "InstanceNorm statistics")
        SC.assert_16bit(ch, SC.instnorm_xhat(c, stats), fl, what + "stored x-hat ch%d" % i)
        if i < 4:
            assert torch.equal(buf["p%d" % i], SC.maxpool2(torch.relu(ch))), what + "p%d != maxpool(relu(ch%d))" % (i, i)
        else:
            SC.assert_16bit(buf["ytok"][:BS], SC.avgpool(torch.relu(ch)), fl, what + "tokens ytok = mean(relu(ch4))")
            assert torch.equal(t.snap["ytok_fwd"][:BS], buf["ytok"][:BS])
    for when, y in (("forward", t.snap["ytok_fwd"]), ("backward", buf["ytok"])):
        assert y.shape[0] == 64 and not bool(y[BS:].any()), t.what + "padding rows of ytok are not zero after the " + when


def head_inputs(t):
    g = t.eng.grid
    return [t.buf["dn"].view(t.B, g, g, 512)] + [t.buf["hu%d" % i] for i in range(3)]


def gn_params(t, i):
    return t.eng.pview("decode_head%d.1.weight" % i), t.eng.pview("decode_head%d.1.bias" % i)


def test_density_head_forward_stages(tr):
    t, buf, eng, fl = tr, tr.buf, tr.eng, tr.fl
    hin = head_inputs(t)
    for i in range(4):
        what = "%sdecode_head%d " % (t.what, i)
        wn, hc = "decode_head%d.0.weight" % i, buf["hc%d" % i]
        cin = hin[i].shape[-1]
        ref = SC.conv3x3(hin[i], eng.Wf[wn].view(256, 3, 3, cin), eng.pview(wn[:-6] + "bias"))
        SC.assert_16bit(hc, ref, fl, what + "conv output hc%d" % i + gemm(t, A=hin[i].data_ptr(), K=9 * cin, modeA=2))
        del ref
        stats = SC.groupnorm_stats(hc)
        SC.assert_stats(buf["hstats%d" % i], stats, what + "GroupNorm statistics")
        ga, be = gn_params(t, i)
        y = SC.groupnorm_relu(hc, stats, ga, be)
        if i < 3:
            hact = t.snap["hact%d" % i].view(hc.shape)
            SC.assert_16bit(hact, y, fl, what + "relu(GroupNorm) in hact_tmp")
            del y
            SC.assert_16bit(buf["hu%d" % i], SC.upsample2x(hact), fl, what + "bilinear x2 hu%d" % i)
        else:
            o1 = SC.head1x1(y, eng.pview("decode_head3.3.weight"), eng.pview("decode_head3.3.bias"))
            del y
            SC.assert_f32(buf["o1"], o1, what + "fused 1x1 head o1")
            o1m = buf["o1"].view(t.B, hc.shape[1], hc.shape[2], 1)
            SC.assert_f32(buf["out"], SC.upsample2x(o1m), what + "bilinear x2 out")


def test_density_head_backward_stages(tr):
    t, buf, eng, fl, B = tr, tr.buf, tr.eng, tr.fl, tr.B
    hin = head_inputs(t)
    side = buf["out"].shape[1] // 2
    d1 = buf["d1"].view(B, side, side)
    SC.assert_f32(buf["d1"], SC.upsample2x_bwd(buf["dout"].unsqueeze(-1)), t.what + "decode_head3 bilinear x2 backward d1")
    for i in (3, 2, 1, 0):
        what = "%sdecode_head%d " % (t.what, i)
        hn, hc = "decode_head%d" % i, buf["hc%d" % i]
        ga, be = gn_params(t, i)
        if i == 3:
            dx, sums, near = SC.groupnorm_relu_bwd(hc, buf["hstats3"], ga, be, d1=d1, w1=eng.pview(hn + ".3.weight"))
            SC.assert_f32(t.grads[hn + ".3.weight"], sums[:, 2].sum(0), what + "gradient of .3.weight")
            SC.assert_f32(t.grads[hn + ".3.bias"], d1.double().sum().reshape(1), what + "gradient of .3.bias")
        else:
            dup = t.snap["dup%d" % (i + 1)].view(B, 2 * hc.shape[1], 2 * hc.shape[2], 256)
            dact = t.snap["dact%d" % i].view(hc.shape)
            SC.assert_16bit(dact, SC.upsample2x_bwd(dup), fl, what + "bilinear x2 backward dact")
            dx, sums, near = SC.groupnorm_relu_bwd(hc, buf["hstats%d" % i], ga, be, dy=dact)
        dpre = t.snap["dpre%d" % i].view(hc.shape)
        SC.assert_16bit(dpre, dx, fl, what + "GroupNorm + ReLU backward dpre", keep=SC.gate_keep(near, what + "ReLU gates"))
        del dx, near
        SC.assert_f32(t.grads[hn + ".1.bias"], sums[:, 0].sum(0), what + "gradient of .1.bias")
        SC.assert_f32(t.grads[hn + ".1.weight"], sums[:, 1].sum(0), what + "gradient of .1.weight")
        cin = hin[i].shape[-1]
        wg = gemm(t, A=eng._ws["dpre"].data_ptr(), K=dpre.numel() // 256, modeB=3)
        SC.assert_f32(t.grads[hn + ".0.weight"], SC.conv3x3_wgrad(dpre, hin[i]), what + "gradient of .0.weight" + wg)
        SC.assert_f32(t.grads[hn + ".0.bias"], SC.bias_grad(dpre), what + "gradient of .0.bias" + wg)
        wd = SC.ohwi_of_dgrad_form(eng.Wd[hn + ".0.weight"], 256, cin)
        got = t.snap["dup%d" % i].view(hin[i].shape) if i else buf["ddn"].view(hin[0].shape)
        dg = gemm(t, A=eng._ws["dpre"].data_ptr(), M=dpre.numel() // 256, modeA=2)
        SC.assert_16bit(got, SC.conv3x3_dgrad(dpre, wd), fl, what + "input gradient " + ("dup" if i else "ddn") + dg)


def test_exemplar_cnn_backward_stages(tr):
    t, buf, eng, fl = tr, tr.buf, tr.eng, tr.fl
    maps = proj_maps(tr)
    SC.assert_16bit(buf["dyt"], buf["dy_tok"].double(), fl, t.what + "dyt = rounded dy_tok")
    for i in (4, 3, 2, 1):
        what = "%sdecoder_proj%d " % (t.what, i)
        wn, ch, dc = "decoder_proj%d.0.weight" % i, buf["ch%d" % i], buf["dc%d" % i]
        dyp = buf["dyt"] if i == 4 else buf["dp%d" % i]
        ref = SC.instnorm_relu_pool_bwd(ch, buf["instats%d" % i][..., 1], dyp, avg=(i == 4))
        SC.assert_16bit(dc, ref, fl, what + "InstanceNorm + ReLU + pool backward dc%d" % i)
        which = " countr_conv3x3_c3_wgrad" if i == 1 else gemm(t, A=dc.data_ptr(), modeB=3)
        SC.assert_f32(t.grads[wn], SC.conv3x3_wgrad(dc, maps[i - 1]), what + "gradient of .0.weight" + which)
        SC.assert_f32(t.grads[wn[:-6] + "bias"], SC.bias_grad(dc), what + "gradient of .0.bias" + which)
        if i > 1:
            wd = SC.ohwi_of_dgrad_form(eng.Wd[wn], PROJ_C[i], PROJ_C[i - 1])
            SC.assert_16bit(buf["dp%d" % (i - 1)], SC.conv3x3_dgrad(dc, wd), fl,
                            what + "input gradient dp%d" % (i - 1) + gemm(t, A=dc.data_ptr(), modeA=2))
