"""Event term of the tracker's camera iteration (SURVEY.md 8 f2 / measurement config 3).

Reference: src/Tracker.py:129-150 (ground-truth event / mask / previous colour image resized with torchvision's
`Resize(NEAREST)`), :150 (`render_img_rescale` of the current pose, with gradient), :153 + src/event_net.py:67-99
(`inference_event`: the two colour images -> `UNet_2heads(6, 2, 2)` -> events * P(event)), :206-228 (L2 event loss,
optionally on Gaussian-blurred images, scaled by `event.balancer`).

The U-Net is a caller-side network and a PyTorch-ROCm module by default (north_star); `compile_event_net` at the end of
this file is its opt-in device route (csrc/event_net.hip: forward and input gradient, frozen eval-mode weights).  It is written here from its
published architecture (5-level U-Net with bilinear up-sampling and two decoder heads) with the parameter names of
the reference checkpoints (event_net/unet_model.py:72-122, event_net/unet_parts.py), so
`pretrained/eventnet_2head_*.pth` loads with `load_state_dict`.  torchvision is not part of this image: the two
torchvision ops on the path are restated on torch primitives --
  Resize(NEAREST) on a tensor   == F.interpolate(mode='nearest')   (source index floor(dst * in/out))
  functional.gaussian_blur(k)   == reflect-pad + depthwise conv with the normalised kernel exp(-x^2 / 2 sigma^2),
                                   sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
and checked against oracle/event_oracle.py (numpy) and scipy.ndimage in tests/test_event_cpu.py."""
import torch
import torch.nn as nn
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------
# torchvision stand-ins (tensor inputs, layout [..., H, W])
# ------------------------------------------------------------------------------------------------
def resize_nearest(img, size):
    """`transforms.Resize(size, InterpolationMode.NEAREST)` of a [C,H,W] (or [H,W]) tensor."""
    x = img
    lead = x.dim()
    while x.dim() < 4:
        x = x[None]
    need_cast = not x.is_floating_point()
    y = F.interpolate(x.float() if need_cast else x, size=tuple(size), mode='nearest')
    if need_cast:
        y = y.to(img.dtype)
    while y.dim() > lead:
        y = y[0]
    return y


def resize_bilinear(img, size):
    """`transforms.Resize(size, InterpolationMode.BILINEAR)` of a [C,H,W] tensor (no antialias: the pinned
    torchvision applies it to tensors only on request)."""
    x = img
    lead = x.dim()
    while x.dim() < 4:
        x = x[None]
    y = F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=False)
    while y.dim() > lead:
        y = y[0]
    return y


def gaussian_kernel1d(kernel_size, sigma=None, dtype=torch.float32, device=None):
    if sigma is None:
        sigma = 0.3 * ((kernel_size - 1) * 0.5 - 1) + 0.8
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size, dtype=dtype, device=device)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur(img, kernel_size, sigma=None):
    """`transforms.functional.gaussian_blur(img, kernel_size)` of a [C,H,W] tensor: separable Gaussian, reflect
    padding, every channel on its own."""
    if kernel_size % 2 != 1 or kernel_size <= 0:
        raise ValueError(f"kernel_size must be odd and positive, got {kernel_size}")
    c, h, w = img.shape
    dt = img.dtype if img.is_floating_point() else torch.float32
    k1 = gaussian_kernel1d(kernel_size, sigma, dtype=dt, device=img.device)
    k2 = torch.outer(k1, k1).expand(c, 1, kernel_size, kernel_size)
    pad = kernel_size // 2
    x = F.pad(img.to(dt)[None], [pad, pad, pad, pad], mode='reflect')
    return F.conv2d(x, k2, groups=c)[0].to(img.dtype)


# ------------------------------------------------------------------------------------------------
# the event network
# ------------------------------------------------------------------------------------------------
class _ConvPair(nn.Module):
    """3x3 conv - BN - ReLU, twice (parameters under `double_conv.{0,1,3,4}`)."""

    def __init__(self, cin, cout, cmid=None):
        super().__init__()
        cmid = cmid or cout
        layers = []
        for a, b in ((cin, cmid), (cmid, cout)):
            layers += [nn.Conv2d(a, b, 3, padding=1, bias=False), nn.BatchNorm2d(b), nn.ReLU(inplace=True)]
        self.double_conv = nn.Sequential(*layers)

    def forward(self, x):
        return self.double_conv(x)


class _Down(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), _ConvPair(cin, cout))

    def forward(self, x):
        return self.maxpool_conv(x)


class _Up(nn.Module):
    """x2 up-sampling of the deep feature, centred zero padding to the skip's size, concat [skip, deep], conv pair."""

    def __init__(self, cin, cout, bilinear=True):
        super().__init__()
        if bilinear:
            self.up = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True)
            self.conv = _ConvPair(cin, cout, cin // 2)
        else:
            self.up = nn.ConvTranspose2d(cin, cin // 2, kernel_size=2, stride=2)
            self.conv = _ConvPair(cin, cout)

    def forward(self, deep, skip):
        deep = self.up(deep)
        dy, dx = skip.shape[2] - deep.shape[2], skip.shape[3] - deep.shape[3]
        if dy or dx:
            deep = F.pad(deep, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
        return self.conv(torch.cat([skip, deep], dim=1))


class _Head(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=1)

    def forward(self, x):
        return self.conv(x)


class UNet_2heads(nn.Module):
    """Shared encoder, two decoders: head 1 regresses the per-polarity event counts, head 2 the probability that a
    pixel fires at all (sigmoid).  `forward(x[B, n_channels, H, W]) -> (events [B, n_classes1, H, W],
    probabilities [B, n_classes2, H, W])` (event_net/unet_model.py:72-122)."""

    WIDTHS = (64, 128, 256, 512, 1024)

    def __init__(self, n_channels, n_classes1, n_classes2, bilinear=True):
        super().__init__()
        self.n_channels, self.n_classes1, self.n_classes2, self.bilinear = n_channels, n_classes1, n_classes2, bilinear
        w = self.WIDTHS
        f = 2 if bilinear else 1
        self.inc = _ConvPair(n_channels, w[0])
        self.down1 = _Down(w[0], w[1])
        self.down2 = _Down(w[1], w[2])
        self.down3 = _Down(w[2], w[3])
        self.down4 = _Down(w[3], w[4] // f)
        for head, ncls in ((1, n_classes1), (2, n_classes2)):         # registration order = the checkpoints' order
            setattr(self, f'up1_{head}', _Up(w[4], w[3] // f, bilinear))
            setattr(self, f'up2_{head}', _Up(w[3], w[2] // f, bilinear))
            setattr(self, f'up3_{head}', _Up(w[2], w[1] // f, bilinear))
            setattr(self, f'up4_{head}', _Up(w[1], w[0], bilinear))
            setattr(self, f'outc_{head}', _Head(w[0], ncls))

    def _decode(self, head, feats):
        x = feats[-1]
        for lvl, skip in zip((1, 2, 3, 4), reversed(feats[:-1])):
            x = getattr(self, f'up{lvl}_{head}')(x, skip)
        return getattr(self, f'outc_{head}')(x)

    def forward(self, x):
        feats = [self.inc(x)]
        for down in (self.down1, self.down2, self.down3, self.down4):
            feats.append(down(feats[-1]))
        return self._decode(1, feats), torch.sigmoid(self._decode(2, feats))


def inference_event(net, img1, img2, device, scale_factor=1, out_threshold=0.5):
    """Predicted event image of the colour pair (img1 = previous, img2 = current; [H,W,3] in [0,1]):
    `(events * P(event))` as [H,W,2] and the probability maps [1,2,H,W] (src/event_net.py:67-99).  Differentiable in
    the images; the network runs in eval mode."""
    net.eval()
    a, b = img1.permute(2, 0, 1), img2.permute(2, 0, 1)
    if a.shape != b.shape:
        raise ValueError('The sizes of the two input images are not the same!')
    if scale_factor != 1.0:
        _, h, w = a.shape
        size = (int(scale_factor * h), int(scale_factor * w))
        if size[0] <= 0 or size[1] <= 0:
            raise ValueError('Scale is too small, resized images would have no pixels')
        a, b = resize_nearest(a, size), resize_nearest(b, size)
    pair = torch.cat((a, b), dim=0)[None].to(device=device, dtype=torch.float32)
    events, probs = net(pair)
    full_events = (events * probs[:, 1][:, None])[0].squeeze().permute(1, 2, 0)
    return full_events, probs


# ------------------------------------------------------------------------------------------------
# the loss
# ------------------------------------------------------------------------------------------------
def event_loss(gt_event, full_event, blur=True, kernel_sizes=(9,), unblurred_weight=0.0, kernel_weights=(1.0,)):
    """Un-balanced event loss of Tracker.py:206-221 on [h,w,2] event images: the L2 distance of the raw images plus
    `kernel_weight` x the L2 distance of their Gaussian-blurred versions.  (`unblurred_weight` only scales the first
    entry of the returned per-term list -- the raw term itself enters the loss with weight 1, exactly like the
    reference.)  Returns (loss, gts_blurred, preds_blurred, term_values)."""
    loss = ((gt_event - full_event) ** 2).sum()
    gts, preds, terms = [], [], [unblurred_weight * loss]
    if blur:
        for k, wk in zip(kernel_sizes, kernel_weights):
            g = gaussian_blur(gt_event.permute(2, 0, 1), k).permute(1, 2, 0)
            p = gaussian_blur(full_event.permute(2, 0, 1), k).permute(1, 2, 0)
            t = ((g - p) ** 2).sum()
            loss = loss + wk * t
            gts.append(g)
            preds.append(p)
            terms.append(t)
    return loss, gts, preds, terms


# ------------------------------------------------------------------------------------------------
# the event network on the device (csrc/event_net.hip): opt-in; the frozen route first, the trainable one after it
# ------------------------------------------------------------------------------------------------
def _conv_pairs(net):
    """The 13 `_ConvPair`s in packing order: inc, down1..4, then per head up1..up4."""
    pairs = [net.inc] + [getattr(net, f'down{i}').maxpool_conv[1] for i in (1, 2, 3, 4)]
    for head in (1, 2):
        pairs += [getattr(net, f'up{lvl}_{head}').conv for lvl in (1, 2, 3, 4)]
    return pairs


def _conv_bn_pairs(net):
    """The 26 (convolution, BatchNorm) pairs in packing order."""
    return [(p.double_conv[i], p.double_conv[i + 1]) for p in _conv_pairs(net) for i in (0, 3)]


def _param_list(net):
    """The 82 parameters in the order of the device entries: per convolution w, gamma, beta; then W1, W2, b1, b2 of the heads."""
    params = [t for conv, bn in _conv_bn_pairs(net) for t in (conv.weight, bn.weight, bn.bias)]
    return params + [net.outc_1.conv.weight, net.outc_2.conv.weight, net.outc_1.conv.bias, net.outc_2.conv.bias]


def _check_input(x, max_batch=1):
    """Raise NotImplementedError unless x is a device tensor [B,6,H >= 16,W >= 16] with 1 <= B <= max_batch."""
    if not x.is_cuda:
        raise NotImplementedError(f"the HIP event network needs its input on a HIP device (got {x.device}); use the torch "
                                  "module on the CPU")
    if max_batch == 1 and (x.dim() != 4 or x.shape[0] != 1):
        raise NotImplementedError(f"the HIP event network runs batch 1 only (got an input of shape {tuple(x.shape)})")
    if x.dim() != 4 or x.shape[1] != 6 or x.shape[2] < 16 or x.shape[3] < 16:
        raise NotImplementedError(f"the HIP event network takes [{1 if max_batch == 1 else 'B'},6,H,W] with H, W >= 16 (got "
                                  f"{tuple(x.shape)})")
    if not 1 <= x.shape[0] <= max_batch:
        raise NotImplementedError(f"the training-mode HIP event network runs batches of 1 to {max_batch} (got "
                                  f"an input of shape {tuple(x.shape)})")


def _cached(cache, key, make):
    """cache[key], made on first use and kept (the per-shape workspaces)."""
    ws = cache.get(key)
    if ws is None:
        ws = cache[key] = make()
    return ws


# (cin, cout) of the 26 convolutions in packing order (EN_CONV of csrc/event_net.hip; the first cin is 6 padded to 8)
EVENTNET_CONVS = ((8, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                  (512, 512)) + ((1024, 512), (512, 256), (512, 256), (256, 128), (256, 128), (128, 64), (128, 64), (64, 64)) * 2
EVENTNET_HEADS_FLOATS = 264


def check_event_net(net, frozen=True, eval_only=True):
    """Raise NotImplementedError unless `net` is what the device route implements: UNet_2heads(6, 2, 2), bilinear, the
    reference's widths, eval mode (`eval_only`; the training-mode route of compile_event_net_batchnorm takes either) and
    (`frozen`, the route of compile_event_net) every parameter frozen."""
    if not isinstance(net, UNet_2heads):
        raise NotImplementedError(f"the HIP event network implements UNet_2heads only, not {type(net).__name__}")
    if not net.bilinear:
        raise NotImplementedError("the HIP event network implements bilinear=True only (no transposed-convolution up-sampling)")
    if (net.n_channels, net.n_classes1, net.n_classes2) != (6, 2, 2):
        raise NotImplementedError("the HIP event network implements UNet_2heads(6, 2, 2) only, got "
                                  f"({net.n_channels}, {net.n_classes1}, {net.n_classes2})")
    got = tuple((c.in_channels, c.out_channels) for c, _ in _conv_bn_pairs(net))
    if got != ((6, 64),) + EVENTNET_CONVS[1:]:
        raise NotImplementedError(f"the HIP event network implements the widths {UNet_2heads.WIDTHS} only")
    if eval_only and net.training:
        raise NotImplementedError("the HIP event network runs eval mode only (BatchNorm folds into the convolutions): call "
                                  "net.eval() first")
    hot = [n for n, p in net.named_parameters() if p.requires_grad] if frozen else []
    if hot:
        raise NotImplementedError(f"{len(hot)} parameters of the event network require gradients (first: {hot[0]}); the HIP "
                                  "route of compile_event_net builds no weight gradients. Freeze the net as the tracker's "
                                  "use implies: net.requires_grad_(False), or train it through compile_event_net_trainable")


def fold_event_net(net):
    """[(w' float64 [cout,cin,3,3], b' float64 [cout])] of the 26 conv + BN pairs in packing order, folded in float64:
    w' = w * gamma / sqrt(var + eps), b' = beta + (conv bias - mean) * gamma / sqrt(var + eps)."""
    out = []
    for conv, bn in _conv_bn_pairs(net):
        w = conv.weight.detach().cpu().double()
        s = bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps)
        shift = -bn.running_mean.detach().cpu().double()
        if conv.bias is not None:
            shift = shift + conv.bias.detach().cpu().double()
        out.append((w * s[:, None, None, None], bn.bias.detach().cpu().double() + shift * s))
    return out


def pack_conv(w, b):
    """One folded convolution (float32 w [cout,cin,3,3], b [cout]) in the kernels' layout: Wf [9 cin'][cout] (row
    tap * cin' + ci, tap = 3 ky + kx, cin' = cin padded to a multiple of 8) | b | Wt [9 cout][cin'] (row tap * cout + co,
    holding w[co, ci, 2 - ky, 2 - kx]: the input gradient is the forward kernel on it)."""
    cout, cin = w.shape[:2]
    if cin % 8:
        w = F.pad(w, [0, 0, 0, 0, 0, 8 - cin % 8])
    wf = w.permute(2, 3, 1, 0).reshape(-1)
    wt = w.flip(2, 3).permute(2, 3, 0, 1).reshape(-1)
    return torch.cat([wf, b, wt])


def pack_event_net(net):
    """The float32 weight image of include/enslam_hip.h (enslam_eventnet_forward), on the CPU: fold in float64, round once."""
    parts = [pack_conv(w.float(), b.float()) for w, b in fold_event_net(net)]
    heads = torch.zeros(EVENTNET_HEADS_FLOATS)
    for h, at_w, at_b in ((1, 0, 256), (2, 128, 258)):
        c = getattr(net, f'outc_{h}').conv
        heads[at_w:at_w + 128] = c.weight.detach().cpu().float().reshape(-1)
        heads[at_b:at_b + 2] = c.bias.detach().cpu().float()
    return torch.cat(parts + [heads]).contiguous()


class HipUNet2Heads(nn.Module):
    """`UNet_2heads.forward` on the device route: `forward(x[1,6,H,W]) -> (events [1,2,H,W], probs [1,2,H,W])`,
    differentiable in x only.  Wraps a frozen eval-mode net (kept as `self.net`); its weights are folded and packed on
    first use and again whenever a parameter or buffer of the net has changed (their `_version`s are remembered), except
    inside a graph capture.  One workspace per (H, W), allocated on first use and kept."""

    def __init__(self, net):
        super().__init__()
        check_event_net(net)
        self.net = net
        self._packed = None
        self._versions = None
        self._workspaces = {}

    def _tensors(self):
        return list(self.net.parameters()) + list(self.net.buffers())

    def _stamp(self):
        return tuple((t.data_ptr(), t._version) for t in self._tensors())

    def packed(self, device):
        from . import functional as EF
        if self._packed is not None and (EF._capturing() or (self._packed.device == device and self._versions == self._stamp())):
            return self._packed
        if EF._capturing():
            raise RuntimeError("HipUNet2Heads: run one call outside the graph capture first (the weights are packed there)")
        check_event_net(self.net)
        stamp = self._stamp()
        self._packed = pack_event_net(self.net).to(device)
        self._versions = stamp
        return self._packed

    def forward(self, x):
        from . import functional as EF
        _check_input(x)
        if self.net.training:
            raise NotImplementedError("the HIP event network runs eval mode only: call .eval()")
        packed = self.packed(x.device)
        key = (int(x.shape[2]), int(x.shape[3]), x.device)
        ws = _cached(self._workspaces, key, lambda: EF.EventNetWorkspace(key[0], key[1], x.device))
        return EF.eventnet_apply(x, packed, ws)


def compile_event_net(net):
    """The device route of a frozen, eval-mode `UNet_2heads(6, 2, 2)`: same call signature and output shapes, so it drops in
    as `slam.event_net` / `inference_event(net=...)`.  Raises NotImplementedError for anything it does not implement."""
    return HipUNet2Heads(net)


# ------------------------------------------------------------------------------------------------
# the trainable route: the packed image is built on the device from the live parameters, autograd carries its gradient
# (csrc/event_net.hip: enslam_eventnet_backward_weights) back through the fold
# ------------------------------------------------------------------------------------------------
def _bn_host_constants(bn):
    """sqrt(running_var + eps) and -running_mean in float64, computed on the host exactly as fold_event_net does."""
    return (torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps), -bn.running_mean.detach().cpu().double())


def pack_event_net_differentiable(net, device=None, constants=None):
    """pack_event_net(net) built on `device` from the live parameters with differentiable torch operations, bit-equal to
    it: sqrt(var + eps) comes from the host in float64 (`constants`: a cached list of _bn_host_constants per conv + BN
    pair, in packing order); the fold itself is fold_event_net's IEEE float64 divide, multiply and add in the same order,
    rounded once to float32; then pack_conv's layout.  The transposed blocks are built without a graph: the image depends
    on a weight through Wf alone, which is where enslam_eventnet_backward_weights puts its gradient."""
    device = torch.device(device) if device is not None else next(net.parameters()).device
    pairs = _conv_bn_pairs(net)
    if constants is None:
        constants = [_bn_host_constants(bn) for _, bn in pairs]
    parts = []
    for (conv, bn), (sq, shift) in zip(pairs, constants):
        sq, shift = sq.to(device), shift.to(device)
        s = bn.weight.to(device).double() / sq
        if conv.bias is not None:
            shift = shift + conv.bias.to(device).double()
        w = (conv.weight.to(device).double() * s[:, None, None, None]).float()
        b = (bn.bias.to(device).double() + shift * s).float()
        if w.shape[1] % 8:
            w = F.pad(w, [0, 0, 0, 0, 0, 8 - w.shape[1] % 8])
        with torch.no_grad():
            wt = w.flip(2, 3).permute(2, 3, 0, 1).reshape(-1)
        parts += [w.permute(2, 3, 1, 0).reshape(-1), b, wt]
    c1, c2 = net.outc_1.conv, net.outc_2.conv
    parts += [c.weight.to(device).float().reshape(-1) for c in (c1, c2)] + [c.bias.to(device).float() for c in (c1, c2)]
    parts.append(torch.zeros(EVENTNET_HEADS_FLOATS - 260, dtype=torch.float32, device=device))
    return torch.cat(parts)


class HipUNet2HeadsTrainable(nn.Module):
    """`UNet_2heads.forward` on the device route with parameter gradients: `forward(x[1,6,H,W]) -> (events, probs)`,
    differentiable in x and in every parameter of `self.net` that requires a gradient (convolution weights, BatchNorm
    gamma and beta, head weights and biases).  The net stays in eval mode: BatchNorm's statistics are frozen and the
    gradients are those of the eval-mode module.  The packed image is rebuilt from the live parameters on every call
    (pack_event_net_differentiable); when no parameter requires a gradient the call is HipUNet2Heads', with no
    weight-gradient launch."""

    def __init__(self, net):
        super().__init__()
        check_event_net(net, frozen=False)
        self.net = net
        self._plain = {}              # the frozen route, a dict so that the net is registered once
        self._constants = None
        self._stamp = None
        self._workspaces = {}

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("the HIP event network runs eval mode only (BatchNorm folds into the convolutions; its "
                                      "statistics stay frozen while the weights train): keep it in .eval()")
        return super().train(mode)

    def _bn_constants(self, device):
        buffers = list(self.net.buffers())
        stamp = (device,) + tuple((t.data_ptr(), t._version) for t in buffers)
        if self._stamp != stamp:
            self._constants = [tuple(t.to(device) for t in _bn_host_constants(bn)) for _, bn in _conv_bn_pairs(self.net)]
            self._stamp = stamp
        return self._constants

    def packed(self, device):
        """The packed image of the live parameters on `device` (with a graph when gradients are enabled): one fused fold on
        the device (csrc/event_net.hip: fold_pack_kernel, bit-equal to pack_event_net, with its own chain rule) when every
        parameter is a contiguous float32 tensor there, pack_event_net_differentiable's torch operations otherwise."""
        from . import functional as EF
        consts = self._bn_constants(device)
        params = _param_list(self.net)
        fused = device.type == 'cuda' and all(conv.bias is None for conv, _ in _conv_bn_pairs(self.net)) and all(
            t.device == device and t.dtype is torch.float32 and t.is_contiguous() for t in params)
        if not fused:
            return pack_event_net_differentiable(self.net, device, consts)
        return EF.eventnet_fold_pack(params, [t for pair in consts for t in pair])

    def forward(self, x):
        from . import functional as EF
        check_event_net(self.net, frozen=False)
        hot = [n for n, p in self.net.named_parameters() if p.requires_grad]
        if not hot:
            if 'net' not in self._plain:
                self._plain['net'] = HipUNet2Heads(self.net)
            return self._plain['net'](x)
        _check_input(x)
        if EF._capturing():
            raise RuntimeError("the trainable HIP event network does not support graph capture of a training step; capture "
                               "the frozen route (compile_event_net) instead")
        key = (int(x.shape[2]), int(x.shape[3]), x.device)
        ws = _cached(self._workspaces, key, lambda: (EF.EventNetWorkspace(key[0], key[1], x.device),
                                                     EF.EventNetTrainScratch(key[0], key[1], x.device)))
        convs_hot = any(not n.startswith('outc_') for n in hot)
        return EF.eventnet_train_apply(x, self.packed(x.device), ws[0], ws[1], convs_hot)


def compile_event_net_trainable(net):
    """The device route of an eval-mode `UNet_2heads(6, 2, 2)` whose parameters may require gradients: same call signature
    and output shapes as the net, `parameters()` / `state_dict()` are the net's own (under `net.`), so
    `torch.optim.Adam(tnet.parameters())` trains it.  Raises NotImplementedError for anything it does not implement."""
    return HipUNet2HeadsTrainable(net)


# ------------------------------------------------------------------------------------------------
# the training-mode route: batch statistics in the forward, their terms in the backward, running statistics updated with
# momentum, mini-batches (csrc/event_net.hip: enslam_eventnet_train_forward / _backward and the three BatchNorm kernels)
# ------------------------------------------------------------------------------------------------
EVENTNET_MAX_BATCH = 8


def check_event_net_batchnorm(net):
    """Raise NotImplementedError unless `net` is what the training-mode device route implements: UNet_2heads(6, 2, 2),
    bilinear, the reference's widths, every BatchNorm affine with tracked running statistics and one momentum and eps."""
    check_event_net(net, frozen=False, eval_only=False)
    bns = [bn for _, bn in _conv_bn_pairs(net)]
    if any(not bn.affine for bn in bns):
        raise NotImplementedError("the training-mode HIP event network implements affine=True BatchNorm only")
    if any(not bn.track_running_stats or bn.running_mean is None for bn in bns):
        raise NotImplementedError("the training-mode HIP event network implements track_running_stats=True only")
    if any(bn.momentum is None for bn in bns):
        raise NotImplementedError("the training-mode HIP event network implements a fixed momentum only (momentum=None, "
                                  "the cumulative average, is not built)")
    if len({(float(bn.momentum), float(bn.eps)) for bn in bns}) != 1:
        raise NotImplementedError("the training-mode HIP event network implements one momentum and eps for all BatchNorms")


class HipUNet2HeadsBatchNorm(nn.Module):
    """`UNet_2heads.forward` on the device route with live BatchNorm.  In training mode `forward(x[B,6,H,W]) -> (events,
    probs)` for 1 <= B <= 8 normalises with the batch statistics, is differentiable in x and in every parameter of
    `self.net` that requires a gradient, and updates running_mean / running_var / num_batches_tracked in place as
    nn.BatchNorm2d does (under torch.no_grad() too).  In eval mode it IS HipUNet2HeadsTrainable on the same net (batch 1),
    which re-folds when the buffers change and so serves the fresh statistics.  `.train()` / `.eval()` reach the net."""

    def __init__(self, net):
        super().__init__()
        check_event_net_batchnorm(net)
        self.net = net
        self.training = net.training
        self._eval = {}               # the eval route, a dict so that the net is registered once
        self._workspaces = {}

    def _params(self):
        return _param_list(self.net), [bn for _, bn in _conv_bn_pairs(self.net)]

    def workspace(self, B, H, W, device):
        """The EventNetBnWorkspace of this input size (allocated on first use and kept)."""
        from . import functional as EF
        key = (int(B), int(H), int(W), torch.device(device))
        return _cached(self._workspaces, key, lambda: EF.EventNetBnWorkspace(*key))

    def forward(self, x):
        from . import functional as EF
        if not self.net.training:
            if 'net' not in self._eval:
                self._eval['net'] = HipUNet2HeadsTrainable(self.net)
            return self._eval['net'](x)
        check_event_net_batchnorm(self.net)
        _check_input(x, EVENTNET_MAX_BATCH)
        B, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
        if EF._capturing():
            raise NotImplementedError("the training-mode HIP event network does not support graph capture of a training step; "
                                      "capture the frozen route (compile_event_net) instead")
        if B * (H // 16) * (W // 16) < 2:                     # the bottom level: torch's own refusal, in its words
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"torch.Size([{B}, 512, {H // 16}, {W // 16}])")
        params, bns = self._params()
        if any(conv.bias is not None for conv, _ in _conv_bn_pairs(self.net)):
            raise NotImplementedError("the training-mode HIP event network implements bias-free convolutions only")
        if any(t.device != x.device or t.dtype is not torch.float32 or not t.is_contiguous() for t in params):
            raise NotImplementedError("the training-mode HIP event network needs contiguous float32 parameters on the input's "
                                      "device")
        buffers = [t for bn in bns for t in (bn.running_mean, bn.running_var)]
        if any(t.device != x.device or t.dtype is not torch.float32 or not t.is_contiguous() for t in buffers):
            raise NotImplementedError("the training-mode HIP event network needs contiguous float32 running statistics on the "
                                      "input's device")
        ws = self.workspace(B, H, W, x.device)
        out = EF.eventnet_bn_net_apply(x, params, ws, float(bns[0].eps), float(bns[0].momentum), buffers)
        for t in buffers:                                     # the kernel wrote them: the eval route re-folds on a new version
            torch.autograd.graph.increment_version(t)
        with torch.no_grad():
            torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)
        return out


def compile_event_net_batchnorm(net):
    """The device route of a `UNet_2heads(6, 2, 2)` with training-mode BatchNorm and mini-batches: same call signature as
    the net, `parameters()` / `buffers()` / `state_dict()` are the net's own (under `net.`), `.train()` / `.eval()` are
    forwarded.  Raises NotImplementedError for anything it does not implement."""
    return HipUNet2HeadsBatchNorm(net)
