"""Network-free event term of the tracker: the contrast-threshold model of event_sim.py predicts the event image between the
previous colour frame and the colour rendered at the pose under optimisation (the event-generation-model loss of the
event-NeRF literature).  Opt-in through `cfg['event']['predictor'] = 'model'`; the default stays the U-Net route.

The model (include/enslam_hip.h states it for the kernel), at the event resolution [h, w]:

    cur [h,w,3]  the rendered colour (carries the gradient)      prev [h,w,3]  the previous ground-truth colour
    gt  [h,w,2]  the recorded event image, channels (-, +)       c_neg, c_pos, eps > 0, K <= 4 Gaussian kernels (k_i odd, w_i)

    Y(a)   = max((0.299 a_R + 0.587 a_G) + 0.114 a_B, 0)
    d      = log(Y(cur) + eps) - log(Y(prev) + eps)
    pred_- = max(-d, 0) / c_neg,   pred_+ = max(d, 0) / c_pos            (d == 0: both 0, gradient 0)
    r      = pred - gt
    loss   = sum r^2 + sum_i w_i sum (B_i r)^2

B_i is `event.gaussian_blur` (separable, reflect padding, per channel, sigma = 0.3 ((k - 1) / 2 - 1) + 0.8).  Blurring is linear,
so one blur of r stands for the two of `event.event_loss`.  As there, the raw term always enters with weight 1 and
`unblurred_weight` only scales the first entry of the reported term list; `blur=False` is K = 0.

    dloss/dr            = 2 r + sum_i 2 w_i B_i^T B_i r          (B^T: the adjoint of the reflect-padded blur, not B)
    d pred_+ / d cur_ch =  [d > 0] w_ch / (c_pos (Y(cur) + eps))
    d pred_- / d cur_ch = -[d < 0] w_ch / (c_neg (Y(cur) + eps))   both zero where Y(cur) was clamped

`predict_events` / `event_model_loss_torch` are that statement in plain torch (any dtype, differentiable, the CPU route);
`EventModelLoss` runs csrc/event_model.hip on a HIP device; `fit_thresholds` estimates c_pos, c_neg of a recorded sequence."""
import torch

from . import event as EV

LUMA = (0.299, 0.587, 0.114)


def _luma(a):
    return torch.clamp((LUMA[0] * a[..., 0] + LUMA[1] * a[..., 1]) + LUMA[2] * a[..., 2], min=0)


def log_luma_difference(cur, prev, eps=1e-3):
    """d [h,w] of the model."""
    return torch.log(_luma(cur) + eps) - torch.log(_luma(prev) + eps)


def predict_events(cur, prev, c_neg=0.2, c_pos=0.2, eps=1e-3):
    """pred [h,w,2] (channels -, +) of colour images cur, prev [h,w,3]; differentiable, any floating dtype."""
    if not (c_neg > 0 and c_pos > 0 and eps > 0):
        raise ValueError(f"c_neg, c_pos and eps must be positive (got {c_neg}, {c_pos}, {eps})")
    d = log_luma_difference(cur, prev, eps)
    return torch.stack((torch.relu(-d) / c_neg, torch.relu(d) / c_pos), dim=-1)


def _kernels(blur, kernel_sizes, kernel_weights):
    if not blur:
        return (), ()
    ks, ws = tuple(int(k) for k in kernel_sizes), tuple(float(x) for x in kernel_weights)
    if len(ks) != len(ws):
        raise ValueError(f"{len(ks)} kernel sizes but {len(ws)} kernel weights")
    return ks, ws


def event_model_loss_torch(cur, prev, gt, c_neg=0.2, c_pos=0.2, eps=1e-3, blur=True, kernel_sizes=(9,), kernel_weights=(1.0,),
                           unblurred_weight=0.0):
    """The model's loss in plain torch: (loss, pred, terms, gts_blurred, preds_blurred) with terms = [unblurred_weight * raw,
    blurred term per kernel] like `event.event_loss`."""
    ks, ws = _kernels(blur, kernel_sizes, kernel_weights)
    pred = predict_events(cur, prev, c_neg, c_pos, eps)
    r = pred - gt
    loss = (r ** 2).sum()
    terms, gts, preds = [unblurred_weight * loss], [], []
    for k, wk in zip(ks, ws):
        if k // 2 >= min(r.shape[0], r.shape[1]):
            raise ValueError(f"kernel size {k} needs reflect padding of {k // 2} >= min(h, w) = {min(r.shape[:2])}")
        t = (EV.gaussian_blur(r.permute(2, 0, 1), k) ** 2).sum()
        loss = loss + wk * t
        terms.append(t)
        with torch.no_grad():
            gts.append(EV.gaussian_blur(gt.permute(2, 0, 1), k).permute(1, 2, 0))
            preds.append(EV.gaussian_blur(pred.detach().permute(2, 0, 1), k).permute(1, 2, 0))
    return loss, pred, terms, gts, preds


class EventModelLoss(torch.autograd.Function):
    """`EventModelLoss.apply(cur, prev, gt, c_neg, c_pos, eps, blur, kernel_sizes, kernel_weights, unblurred_weight,
    want_blurred)` -> (loss, pred, terms, gts_blurred, preds_blurred), differentiable in cur through loss only (the last three
    are lists of detached tensors).  On a HIP device: one call of enslam_event_model_loss (float32 images; loss and terms float64 0-d tensors), whose unit gradient the
    backward scales by the incoming scalar; no host synchronisation, so it can be recorded in a hipGraph.  On CPU tensors: the
    torch statement above.  gts_blurred / preds_blurred hold [h,w,2] images and are empty without `want_blurred`."""

    @staticmethod
    def forward(ctx, cur, prev, gt, c_neg=0.2, c_pos=0.2, eps=1e-3, blur=True, kernel_sizes=(9,), kernel_weights=(1.0,),
                unblurred_weight=0.0, want_blurred=True):
        ks, ws = _kernels(blur, kernel_sizes, kernel_weights)
        if cur.is_cuda:
            from . import functional as EF
            c = EF._f32c(cur)
            pred, sums, grad, bg, bp = EF.event_model_loss(c, EF._f32c(prev), EF._f32c(gt), c_neg, c_pos, eps, ks, ws, want_blurred)
            ctx.unit = grad
            ctx.cur_dtype = cur.dtype
            loss = sums[len(ks) + 1]
            terms = (sums[0] * unblurred_weight,) + tuple(sums[1 + i] for i in range(len(ks)))
            gts = tuple(bg[i] for i in range(len(ks))) if bg is not None else ()
            preds = tuple(bp[i] for i in range(len(ks))) if bp is not None else ()
        else:
            with torch.enable_grad():
                leaf = cur.detach().requires_grad_(True)
                loss_g, pred, terms, gts, preds = event_model_loss_torch(leaf, prev.detach(), gt.detach(), c_neg, c_pos, eps, blur, ks,
                                                                         ws, unblurred_weight)
                ctx.unit, = torch.autograd.grad(loss_g, leaf)
            ctx.cur_dtype = cur.dtype
            loss, pred = loss_g.detach(), pred.detach()
            terms, gts, preds = tuple(t.detach() for t in terms), tuple(gts), tuple(preds)
            if not want_blurred:
                gts = preds = ()
        ctx.mark_non_differentiable(pred)
        ctx.set_materialize_grads(False)
        return loss, pred, list(terms), list(gts), list(preds)         # (lists pass through autograd as they are: no graph)

    @staticmethod
    def backward(ctx, g_loss, *_unused):
        if g_loss is None:
            return (None,) * 11
        return ((ctx.unit * g_loss.to(ctx.unit.dtype)).to(ctx.cur_dtype),) + (None,) * 10


def event_model_loss(cur, prev, gt, c_neg=0.2, c_pos=0.2, eps=1e-3, blur=True, kernel_sizes=(9,), kernel_weights=(1.0,),
                     unblurred_weight=0.0, want_blurred=True):
    """`EventModelLoss.apply` with keyword arguments and defaults."""
    return EventModelLoss.apply(cur, prev, gt, c_neg, c_pos, eps, blur, tuple(kernel_sizes), tuple(kernel_weights), unblurred_weight,
                                want_blurred)


def fit_thresholds(pairs, eps=1e-3):
    """Least-squares contrast thresholds of a recorded sequence: `pairs` yields (prev colour [h,w,3], cur colour [h,w,3], event
    image [h,w,2] with channels -, +).  With d the model's log-luminance difference, 1 / c_+ = sum d+ n+ / sum (d+)^2 over the
    pixels with d > 0 and likewise 1 / c_- over d < 0 (float64 sums).  Returns dict(c_pos, c_neg, n_pos, n_neg); a side with no
    signal (sum d n <= 0) gives None.  Counts are floored by a sensor, which biases the estimate towards larger thresholds."""
    s = torch.zeros(4, dtype=torch.float64)
    n_pos = n_neg = 0
    for prev, cur, ev in pairs:
        d = log_luma_difference(cur.double(), prev.double(), eps)
        dp, dn, ev = torch.relu(d), torch.relu(-d), ev.double()
        s += torch.stack(((dp * ev[..., 1]).sum(), (dp * dp).sum(), (dn * ev[..., 0]).sum(), (dn * dn).sum())).cpu()
        n_pos += int((d > 0).sum())
        n_neg += int((d < 0).sum())
    s = s.tolist()
    return dict(c_pos=s[1] / s[0] if s[0] > 0 else None, c_neg=s[3] / s[2] if s[2] > 0 else None, n_pos=n_pos, n_neg=n_neg)
