"""Training-side pieces (SURVEY s.8f row N4) on the GPU, through the C ABI: Dice loss value + gradient against the fixture made
from the reference's own DiceLoss, the fused sigmoid/clip chain against torch autograd, AdamW against torch.optim.AdamW, and
a short optimisation loop built from the two against the same loop on the CPU oracle."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_dice_loss_matches_reference_fixture(gpu, gold):
    from cryovit_amd.models import DiceLoss

    g = gold("train_pieces.npz")
    probs = torch.from_numpy(g["dice_probs"]).to(gpu).requires_grad_(True)
    labels = torch.from_numpy(g["dice_labels"]).to(gpu)  # int8, -1 = ignore: masked inside the kernel
    loss = DiceLoss()(probs, labels)
    assert abs(float(loss.detach()) - float(g["dice_loss"])) <= 2e-6  # fp32 sums in a different (fixed) order
    (3.0 * loss).backward()
    want = 3.0 * torch.from_numpy(g["dice_grad"])
    assert torch.allclose(probs.grad.cpu(), want, rtol=2e-5, atol=1e-9)
    assert torch.all(probs.grad[labels < 0] == 0)
    # the reference's call shape: masked vectors [n, 1] with float labels
    m = labels > -1
    yp = torch.masked_select(probs.detach(), m).view(-1, 1).requires_grad_(True)
    loss2 = DiceLoss()(yp, torch.masked_select(labels, m).view(-1, 1).float())
    assert abs(float(loss2) - float(g["dice_loss"])) <= 2e-6
    loss2.backward()
    assert torch.allclose(yp.grad.view(-1).cpu(), torch.from_numpy(g["dice_grad"])[m.cpu()], rtol=2e-5, atol=1e-9)
    # bitwise reproducible (no atomics)
    outs = [float(DiceLoss()(probs.detach(), labels)) for _ in range(3)]
    assert outs[0] == outs[1] == outs[2]


@pytest.mark.parametrize("n", [1, 3, 1026, 1 << 20, 33554432 // 8 + 5])
def test_dice_loss_sizes_and_logit_chain(gpu, n):
    """Ragged sizes (n % 4 != 0, fewer elements than one block, more than CVX_DICE_BLOCKS blocks' worth) and the fused
    d loss / d logit through p = sigmoid(clip(x, -5, 5)) against torch autograd of the oracle expression."""
    from cryovit_amd.models.losses import dice_loss_and_logit_grad
    from oracle import train_pieces as tp

    gen = torch.Generator().manual_seed(n % 1000)
    raw = torch.randn(n, generator=gen) * 4.0  # a good share beyond the +-5 clip
    labels = torch.randint(-1, 2, (n,), generator=gen)
    x = raw.clone().requires_grad_(True)
    clipped = torch.clip(x, -5.0, 5.0)
    probs = torch.sigmoid(clipped)
    ref = tp.masked_dice_loss(probs.double(), labels.double())
    ref.backward()
    loss, grad = dice_loss_and_logit_grad(probs.detach().to(gpu), clipped.detach().to(gpu), labels.to(torch.int8).to(gpu), 1.0)
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    inside = raw.abs() < 5.0
    assert torch.allclose(grad.cpu()[inside], x.grad[inside].float(), rtol=1e-4, atol=1e-12 + 1e-4 * float(x.grad.abs().max()))
    assert torch.all(grad.cpu()[~inside] == 0)


@pytest.mark.parametrize("n,kw", [(8401737, dict(lr=1e-4, weight_decay=1e-2)), (1027, dict(lr=3e-3, weight_decay=0.0, betas=(0.8, 0.95), eps=1e-6)),
                                  (2, dict(lr=1e-2, weight_decay=0.1))])
def test_adamw_matches_torch(gpu, n, kw):
    """cvx_adamw_step against torch.optim.AdamW (CPU, single-tensor path) over 6 steps; n = the head's parameter count, a
    ragged size and a tiny one.  Same operations in the same order; hipcc contracts a*b+c into one FMA where torch rounds
    twice, hence a few ulp instead of bit equality."""
    from cryovit_amd.engine import ops

    gen = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, generator=gen)
    ref_p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref_p], foreach=False, **kw)
    b1, b2 = kw.get("betas", (0.9, 0.999))
    p, m, v = p0.to(gpu), torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    for step in range(1, 7):
        g = torch.randn(n, generator=gen) * (0.1 if step % 2 else 3.0)
        ref_p.grad = g.clone()
        opt.step()
        ops.adamw_step(p, g.to(gpu), m, v, lr=kw["lr"], beta1=b1, beta2=b2, eps=kw.get("eps", 1e-8), weight_decay=kw["weight_decay"], step=step)
    assert torch.allclose(p.cpu(), ref_p.detach(), rtol=2e-6, atol=2e-7), float((p.cpu() - ref_p.detach()).abs().max())
    st = opt.state[ref_p]
    # (the moments: values near zero after cancellation between steps carry the absolute round-off of their O(1) terms)
    assert torch.allclose(m.cpu(), st["exp_avg"], rtol=2e-6, atol=1e-6) and torch.allclose(v.cpu(), st["exp_avg_sq"], rtol=4e-6, atol=1e-8)


def test_optimisation_loop_dice_plus_adamw(gpu):
    """The two pieces together: a bias volume added to fixed logits is trained with DiceLoss + the fused AdamW (parameters
    re-pointed into the flat buffers, gradients accumulated in place); the loss trajectory follows the CPU loop built from the
    oracle's Dice loss and torch.optim.AdamW, and goes down."""
    from cryovit_amd.models import DiceLoss
    from cryovit_amd.training.optim import AdamW
    from oracle import train_pieces as tp

    gen = torch.Generator().manual_seed(21)
    base = torch.randn(4, 24, 40, generator=gen)
    labels = (torch.rand(4, 24, 40, generator=gen) < 0.3).float()
    labels[0] = -1.0
    w_gpu = [torch.nn.Parameter(torch.zeros(4, 24, 40, device=gpu)), torch.nn.Parameter(torch.zeros(3, device=gpu))]  # (+ an odd-sized tensor)
    w_cpu = [torch.nn.Parameter(torch.zeros(4, 24, 40)), torch.nn.Parameter(torch.zeros(3))]
    opt_g, opt_c = AdamW(w_gpu, lr=5e-2, weight_decay=1e-2), torch.optim.AdamW(w_cpu, lr=5e-2, weight_decay=1e-2, foreach=False)
    loss_fn = DiceLoss()
    lg, lc = [], []
    for _ in range(12):
        opt_g.zero_grad()
        pg = torch.sigmoid(torch.clip(base.to(gpu) + w_gpu[0] + w_gpu[1].sum(), -5.0, 5.0))
        loss = loss_fn(pg, labels.to(gpu))
        loss.backward()
        opt_g.step()
        lg.append(float(loss))
        opt_c.zero_grad()
        pc = torch.sigmoid(torch.clip(base + w_cpu[0] + w_cpu[1].sum(), -5.0, 5.0))
        loss_c = tp.masked_dice_loss(pc, labels)
        loss_c.backward()
        opt_c.step()
        lc.append(float(loss_c))
    assert np.allclose(lg, lc, rtol=2e-4, atol=2e-5), (lg, lc)
    assert lg[-1] < lg[0] - 0.05
    assert torch.allclose(w_gpu[0].detach().cpu(), w_cpu[0].detach(), atol=2e-3)
    assert w_gpu[0].data_ptr() == opt_g.flat_p.data_ptr()  # the parameter IS a view of the flat buffer


def test_adamw_stays_attached_or_raises(gpu):
    """Gradients dropped by ``zero_grad(set_to_none=True)`` are re-attached to the flat buffer (the step still sees what
    autograd then accumulates); a parameter or gradient that moved away from its slice is an error, not a silent no-op; the
    state dict carries the flat layout and a foreign one is refused."""
    from cryovit_amd.training.optim import AdamW

    lin = torch.nn.Linear(5, 3).to(gpu)
    opt = AdamW(lin.parameters(), lr=1e-1, weight_decay=0.0)
    x = torch.randn(7, 5, device=gpu)
    lin.zero_grad(set_to_none=True)          # torch's default: .grad = None
    opt.step()                               # re-attaches, steps with zero gradients: parameters unchanged
    assert all(p.grad is not None and p.grad.data_ptr() == opt.flat_g.data_ptr() + o * 4 for p, o in zip(opt.params, opt.offsets))
    before = opt.flat_p.clone()
    lin(x).square().sum().backward()         # accumulates into the re-attached slices
    assert float(opt.flat_g.abs().sum()) > 0
    opt.step()
    assert not torch.equal(opt.flat_p, before)
    sd = opt.state_dict()
    assert sd["n"] == opt.n and sd["offsets"] == opt.offsets
    opt.load_state_dict(sd)
    other = AdamW(torch.nn.Linear(5, 4).to(gpu).parameters())
    with pytest.raises(ValueError):
        other.load_state_dict(sd)
    lin.weight.grad = torch.zeros_like(lin.weight)  # a replaced gradient tensor
    with pytest.raises(RuntimeError):
        opt.step()
    lin.weight.grad = None
    lin.weight.data = lin.weight.data.clone()       # a moved parameter (model.to(), assign=True load ...)
    with pytest.raises(RuntimeError):
        opt.step()


def _focal_operands(saturated):
    """test_focal_loss_against_oracle's input; ``saturated`` appends x in +-{10, 17, 30, 100}, each with label 0 and label 1."""
    gen = torch.Generator().manual_seed(31)
    n = 50021
    x = torch.rand(n, generator=gen)            # the reference feeds probabilities
    x[:100] = torch.randn(100, generator=gen) * 4  # ... and the formula must hold for any real input
    labels = torch.randint(-1, 2, (n,), generator=gen)
    if saturated:
        x = torch.cat([x, torch.tensor([s * v for v in (10.0, 17.0, 30.0, 100.0) for s in (1, -1) for _ in (0, 1)])])
        labels = torch.cat([labels, torch.tensor([0, 1] * 8)])
    return x, labels


def _focal_oracle(x, labels, gamma):
    """(loss, d loss / d x) of the float64 oracle over labels > -1.  Where the prediction is right beyond float64 -- 1 - p_t == 0
    exactly, |x| > 36.7 -- autograd of ``(1 - p_t) ** gamma`` yields inf * 0 = NaN for gamma < 1; the derivative there is
    alpha_t d/dx [m^gamma ce] with m = sigmoid(-|x|) and ce = log1p(exp(-|x|)) <= m, below (1 + gamma) exp(-36.7)^(1 + gamma) < 1e-15 of
    the O(1) gradients of the set: 0 at every tolerance used here.  Those NaNs (and only those) are replaced by 0."""
    from oracle import train_pieces as tp

    m = labels > -1
    xr = x.double().clone().requires_grad_(True)
    ref = tp.focal_loss(xr[m], labels[m].double(), gamma=gamma)
    ref.backward()
    grad = xr.grad.clone()
    bad = torch.isnan(grad)
    if bool(bad.any()):
        assert gamma < 1 and bool(((x.abs() > 36.7) & m & ((x > 0) == (labels == 1)))[bad].all())
        grad[bad] = 0.0
    return float(ref.detach()), grad


@pytest.mark.parametrize("gamma", [0, 0.5, 1, 3])
def test_focal_loss_gamma_branches_and_saturated_inputs(gpu, gamma):
    """The kernel's gamma == 0 branch (plain weighted cross-entropy), its ``powf`` path below and above 1 (0.5: m^(gamma - 1) grows
    without bound as m -> 0 and is floored at m = 1e-30; 1; 3) beside the existing 2 and 1.5, on the existing input plus a block of
    saturated values x in +-{10, 17, 30, 100} with both labels (sigmoid rounds to 0 / 1 in fp32 from |x| = 17 on).  Tolerances of
    test_focal_loss_against_oracle.  They hold for the saturated block on the CPU: the oracle's formula evaluated in fp32 against its
    float64 self on this input is off by at most 0.007 of the gradient tolerance (x = 17, label 0, gamma 3) and 2.7e-8 relative in
    the loss (gamma 0), so no wider band is taken for it."""
    from cryovit_amd.models.losses import FocalLoss

    x, labels = _focal_operands(saturated=True)
    ref, grad = _focal_oracle(x, labels, gamma)
    xg = x.to(gpu).requires_grad_(True)
    loss = FocalLoss(gamma=gamma)(xg, labels.to(gpu))
    print(f"focal gamma={gamma}: loss {float(loss.detach())!r} oracle {ref!r}")
    assert abs(float(loss.detach()) - ref) <= 2e-6 * max(1.0, abs(ref))
    (2.0 * loss).backward()
    want = 2.0 * grad.float()
    got = xg.grad.cpu()
    assert not bool(torch.isnan(got).any())
    tol = 2e-4 * want.abs() + 1e-9 + 2e-6 * float(want.abs().max())
    print(f"focal gamma={gamma}: max gradient error / tolerance {float(((got - want).abs() / tol).max()):.3f}")
    assert torch.allclose(got, want, rtol=2e-4, atol=1e-9 + 2e-6 * float(want.abs().max()))
    assert torch.all(xg.grad[labels.to(gpu) < 0] == 0)


@pytest.mark.parametrize("gamma", [2, 0.5])
def test_focal_loss_one_class_and_no_label(gpu, gamma):
    """alpha = (n - sum y) / n at its ends.  Every labelled voxel a 1: alpha = 0, the positives' weight, so loss and gradient are
    exactly 0.  Every labelled voxel a 0: alpha = 1, the oracle's value and gradient.  Every voxel ignored: loss 0, gradient 0, no NaN
    (the kernel's ``cnt > 0`` guards; the reference divides 0 by 0 there)."""
    from cryovit_amd.models.losses import FocalLoss

    x, labels = _focal_operands(saturated=True)
    keep = labels > -1
    for fill in (1, 0, -1):
        lab = torch.where(keep, torch.full_like(labels, fill), labels) if fill > -1 else torch.full_like(labels, -1)
        xg = x.to(gpu).requires_grad_(True)
        loss = FocalLoss(gamma=gamma)(xg, lab.to(gpu))
        (2.0 * loss).backward()
        got = xg.grad.cpu()
        assert not bool(torch.isnan(got).any()) and torch.all(got[lab < 0] == 0)
        if fill == 0:
            ref, grad = _focal_oracle(x, lab, gamma)
            want = 2.0 * grad.float()
            assert abs(float(loss.detach()) - ref) <= 2e-6 * max(1.0, abs(ref))
            assert torch.allclose(got, want, rtol=2e-4, atol=1e-9 + 2e-6 * float(want.abs().max()))
        else:
            assert float(loss.detach()) == 0.0 and torch.all(got == 0), fill


def test_dice_loss_every_label_ignored(gpu):
    """No labelled voxel: the sums are 0, the loss is exactly 1 - 0 / 1e-3 = 1, and the gradient is zero everywhere, in the plain
    form and through the sigmoid (with and without the clipped logits)."""
    from cryovit_amd.engine import ops
    from cryovit_amd.models import DiceLoss
    from cryovit_amd.models.losses import dice_loss_and_logit_grad

    n = 4099
    raw = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000)) * 4.0  # a good share beyond the +-5 clip
    clipped = torch.clip(raw, -5.0, 5.0)
    probs = torch.sigmoid(clipped).to(gpu)
    labels = torch.full((n,), -1, dtype=torch.int8, device=gpu)
    out4 = torch.full((4,), -77.0, device=gpu)
    ops.dice_loss_forward(probs, labels, out4)
    assert out4.cpu().tolist() == [0.0, 0.0, 0.0, 1.0]
    pg = probs.clone().requires_grad_(True)
    loss = DiceLoss()(pg, labels)
    assert float(loss.detach()) == 1.0
    (3.0 * loss).backward()
    assert torch.all(pg.grad == 0)
    for lg in (clipped.to(gpu), None):
        loss, grad = dice_loss_and_logit_grad(probs, lg, labels, 3.0)
        assert float(loss) == 1.0 and torch.all(grad == 0) and grad.shape == probs.shape


def test_dice_loss_empty_selection(gpu):
    """The reference's call shape on a crop without a labelled voxel: ``masked_select`` leaves [0, 1] tensors.  The formula gives
    1 - 0 / (0 + 1e-3) = 1 and an empty gradient (checked on the oracle here, too)."""
    from cryovit_amd.models import DiceLoss
    from oracle import train_pieces as tp

    probs = torch.rand(4, 6, 5, generator=torch.Generator().manual_seed(3))
    labels = torch.full((4, 6, 5), -1.0)
    m = labels > -1
    yr = torch.masked_select(probs, m).view(-1, 1).requires_grad_(True)
    ref = tp.dice_loss(yr, torch.masked_select(labels, m).view(-1, 1))
    ref.backward()
    assert float(ref) == 1.0 and tuple(yr.grad.shape) == (0, 1)
    yp = torch.masked_select(probs.to(gpu), m.to(gpu)).view(-1, 1).requires_grad_(True)
    loss = DiceLoss()(yp, torch.masked_select(labels.to(gpu), m.to(gpu)).view(-1, 1))
    assert float(loss.detach()) == 1.0
    loss.backward()
    assert tuple(yp.grad.shape) == (0, 1) and yp.grad.dtype == torch.float32


@pytest.mark.parametrize("n", [3, 1026, 70001])
def test_dice_loss_logit_grad_without_logits(gpu, n):
    """``dice_loss_and_logit_grad(probs, None, ...)``: without the stored logits there is no clip to see, the gradient is the chain
    through the sigmoid alone, d loss / d p * p (1 - p), at every voxel -- against autograd of the oracle expression (float64) with
    the tolerances of test_dice_loss_sizes_and_logit_chain."""
    from cryovit_amd.models.losses import dice_loss_and_logit_grad
    from oracle import train_pieces as tp

    gen = torch.Generator().manual_seed(n % 1000)
    raw = torch.randn(n, generator=gen) * 4.0
    labels = torch.randint(-1, 2, (n,), generator=gen)
    probs = torch.sigmoid(torch.clip(raw, -5.0, 5.0))  # fp32, as the head stores them
    z = torch.logit(probs.double()).requires_grad_(True)  # the pre-sigmoid value OF THE STORED probability
    ref = tp.masked_dice_loss(torch.sigmoid(z), labels.double())
    ref.backward()
    loss, grad = dice_loss_and_logit_grad(probs.to(gpu), None, labels.to(torch.int8).to(gpu), 1.0)
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    want = z.grad.float()
    assert torch.allclose(grad.cpu(), want, rtol=1e-4, atol=1e-12 + 1e-4 * float(want.abs().max()))
    assert torch.all(grad.cpu()[labels < 0] == 0)


@pytest.mark.parametrize("gamma", [2, 1.5])
def test_focal_loss_against_oracle(gpu, gamma):
    """FocalLoss (losses.py:35-64) against the oracle restatement of torchvision's sigmoid_focal_loss (float64): value and autograd
    gradient, masked in the kernel; alpha = (n - sum y) / n is a constant of the gradient like the reference's weight.item()."""
    from cryovit_amd.models.losses import FocalLoss
    from oracle import train_pieces as tp

    gen = torch.Generator().manual_seed(31)
    n = 50021
    x = torch.rand(n, generator=gen)            # the reference feeds probabilities
    x[:100] = torch.randn(100, generator=gen) * 4  # ... and the formula must hold for any real input
    labels = torch.randint(-1, 2, (n,), generator=gen)
    m = labels > -1
    xr = x.double().clone().requires_grad_(True)
    ref = tp.focal_loss(xr[m], labels[m].double(), gamma=gamma)
    ref.backward()
    xg = x.to(gpu).requires_grad_(True)
    loss = FocalLoss(gamma=gamma)(xg, labels.to(gpu))
    assert abs(float(loss.detach()) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref)))
    (2.0 * loss).backward()
    want = 2.0 * xr.grad.float()
    assert torch.allclose(xg.grad.cpu(), want, rtol=2e-4, atol=1e-9 + 2e-6 * float(want.abs().max()))
    assert torch.all(xg.grad[labels.to(gpu) < 0] == 0)
