"""Wiring defects an engine could carry, applied to the ORACLE (CPU, fp32) so that their size can be measured without a GPU.

Each mutant is a context manager `mutant(nets, inp)`: nets = (tryon unet, garment unet, vae) of `parity_utils.build(...)["oracle"]`, inp = the
dict of `parity_utils.make_inputs`.  Inside the `with` the oracle (or its inputs) carries the defect; on exit everything is as it was.  The
docstring names the engine defect the mutant stands for.  `oracle/` itself stays a clean restatement: all patching lives here.  Nothing in
this module touches the engine or runs on a GPU -- tests/test_parity_audit_cpu.py uses it to show that the model-level bars of
tests/parity_checks.py can hear each of these defects on the "loud" weights of tests/parity_utils.py.

`oracle.layers.sdpa` is looked up as a module global by both attention processors, and `oracle.pipeline.run` looks up `denoise` the same way, so
replacing the attribute is enough.  The VAE and the Resampler have their own attention code and are not mutated.
"""
import contextlib
import math

import torch

from oracle import layers as L
from oracle import pipeline as opipe
from oracle import unet as U


@contextlib.contextmanager
def _attr(obj, name, value):
    """setattr for the duration; an attribute that lived only on the class is removed from the instance again."""
    own = name in vars(obj) if hasattr(obj, "__dict__") else True
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        if own:
            setattr(obj, name, old)
        else:
            delattr(obj, name)


# ------------------------------------------------------------------------------------------------------------------------------------
# attention arithmetic: replace oracle.layers.sdpa
# ------------------------------------------------------------------------------------------------------------------------------------
def _softmax_qk(q, k, scale=None):
    return torch.softmax((q @ k.transpose(-2, -1)) * (q.shape[-1] ** -0.5 if scale is None else scale), dim=-1)


def log2e_scale(nets, inp):
    """The softmax scale folded with log2(e) for an exp2-based softmax, and the kernel then calling exp: every logit 1.44x too large."""
    return _attr(L, "sdpa", lambda q, k, v: _softmax_qk(q, k, q.shape[-1] ** -0.5 * math.log2(math.e)) @ v)


def uniform(nets, inp):
    """Logits lost (a zeroed or unwritten S tile): every query gets the mean of V."""
    return _attr(L, "sdpa", lambda q, k, v: v.mean(dim=-2, keepdim=True).expand(*q.shape[:-1], v.shape[-1]))


def v_key_order_only(nets, inp):
    """V^T stored in the attention kernel's key order (ops.key_order) while the probabilities come in plain key order: inside each whole
    group of 16 keys, P meets the wrong V rows.  A trailing partial group is left in place."""
    from idm_vton_amd import ops

    def sdpa(q, k, v):
        n = v.shape[-2] // 16 * 16
        idx = torch.cat([ops.key_order_index(n), torch.arange(n, v.shape[-2])])
        return _softmax_qk(q, k) @ v.index_select(-2, idx)
    return _attr(L, "sdpa", sdpa)


def unmasked_pad_keys(nets, inp):
    """The filler rows that pad a key count to a multiple of 16 take part in the softmax: round16(N) - N zero keys and zero values appended
    (logit 0, value 0).  Where N is already a multiple of 16, 5 are appended, so that sizes without filler rows hear the same defect."""
    def sdpa(q, k, v):
        n = k.shape[-2]
        pad = (-n) % 16 or 5
        z = lambda t: torch.cat([t, t.new_zeros(*t.shape[:-2], pad, t.shape[-1])], dim=-2)
        return _softmax_qk(q, z(k)) @ z(v)
    return _attr(L, "sdpa", sdpa)


def unmasked_self_filler(nets, inp):
    """The narrow form of `unmasked_pad_keys`, for sizes whose token count T is no multiple of 16 (320x320: T = 100 at the coarsest level): the
    engine keeps round16(T) token rows per image, and only the self-attentions see those filler rows as keys -- once in GarmentNet, twice
    (person and garment segment) in TryonNet.  That many zero keys and values appended there and nowhere else; no effect where T % 16 == 0."""
    def sdpa(q, k, v):
        tq, n = q.shape[-2], k.shape[-2]
        pad = n // tq * ((-tq) % 16) if n in (tq, 2 * tq) else 0
        z = lambda t: torch.cat([t, t.new_zeros(*t.shape[:-2], pad, t.shape[-1])], dim=-2)
        return _softmax_qk(q, z(k)) @ z(v)
    return _attr(L, "sdpa", sdpa)


# ------------------------------------------------------------------------------------------------------------------------------------
# self-attention with the garment: what `garment_features[idx]` hands a TryonNet block
# ------------------------------------------------------------------------------------------------------------------------------------
class _Features:
    """Stands in for the garment feature list: indexing goes through `pick(features, idx)`."""

    def __init__(self, feats, pick):
        self.feats, self.pick = feats, pick

    def __getitem__(self, idx):
        return self.pick(self.feats, idx)

    def __len__(self):
        return len(self.feats)


def _garment(pick):
    orig = U.BasicTransformerBlock.forward

    def forward(self, x, encoder_hidden_states, garment_features=None, idx=0):
        if self.mode == "tryon":
            garment_features = _Features(garment_features, pick)
        return orig(self, x, encoder_hidden_states, garment_features, idx)
    return _attr(U.BasicTransformerBlock, "forward", forward)


def garment_next_block(nets, inp):
    """The feature cursor one ahead: block i attends to the garment feature of block i+1 wherever the two have the same shape."""
    return _garment(lambda f, i: f[i + 1] if i + 1 < len(f) and f[i + 1].shape == f[i].shape else f[i])


def uncond_sees_garment(nets, inp):
    """The closed-form zero segment of the unconditional half missing: both CFG halves attend to the garment."""
    return _garment(lambda f, i: torch.cat([f[i][f[i].shape[0] // 2:]] * 2))


def garment_tail_dropped(nets, inp):
    """The last tile of garment keys not visited (a tile count one short): the last 16 garment keys are missing."""
    return _garment(lambda f, i: f[i][:, :-16])


def garments_swapped(nets, inp):
    """The garment index reversed within the batch: person b attends to garment B-1-b (needs B >= 2)."""
    def pick(f, i):
        g = f[i]
        b = g.shape[0] // 2
        return torch.cat([g[:b], g[b:].flip(0)])
    return _garment(pick)


# ------------------------------------------------------------------------------------------------------------------------------------
# GarmentNet
# ------------------------------------------------------------------------------------------------------------------------------------
def cloth_text_ignored(nets, inp):
    """GarmentNet's cross-attention context never filled: it attends to zeros instead of the cloth caption."""
    o_g = nets[1]
    orig = o_g.forward
    return _attr(o_g, "forward", lambda z, t, txt, **kw: orig(z, t, torch.zeros_like(txt), **kw))


def timestep_stale(nets, inp):
    """The garment features of the first step reused (or its time-embedding row read) on every step: GarmentNet sees the first step's t."""
    orig = opipe.denoise

    def denoise(unet, unet_encoder, sched, timesteps, *a, **kw):
        t0 = timesteps[0]
        return orig(unet, lambda z, t, txt: unet_encoder(z, t0, txt), sched, timesteps, *a, **kw)
    return _attr(opipe, "denoise", denoise)


# ------------------------------------------------------------------------------------------------------------------------------------
# cross-attention
# ------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _ip_processors(nets, name, value):
    procs = [m for m in nets[0].modules() if isinstance(m, L.IPAttnProcessor2_0)]
    old = [getattr(p, name) for p in procs]
    for p in procs:
        setattr(p, name, value)
    try:
        yield
    finally:
        for p, o in zip(procs, old):
            setattr(p, name, o)


def ip_scale_zero(nets, inp):
    """The image-prompt branch of the cross-attention dropped (scale 0): text attention alone."""
    return _ip_processors(nets, "scale", 0.0)


def ip_split_at_4(nets, inp):
    """The text / image-token split at the IP-Adapter default of 4 tokens instead of the 16 this model uses: 12 image tokens join the text
    keys."""
    return _ip_processors(nets, "num_tokens", 4)


@contextlib.contextmanager
def _inputs(inp, **new):
    old = {k: inp[k] for k in new}
    inp.update(new)
    try:
        yield
    finally:
        inp.update(old)


def ip_rows_swapped(nets, inp):
    """The two halves of `ip_hidden_states` ([uncond ; cond]) taken the other way round: the conditional half sees the blank image."""
    x = inp["ip_hidden_states"]
    b = x.shape[0] // 2
    return _inputs(inp, ip_hidden_states=torch.cat([x[b:], x[:b]]))


def prompt_negative_swapped(nets, inp):
    """[negative ; prompt] concatenated as [prompt ; negative]: each CFG half attends to the other's text."""
    return _inputs(inp, prompt_embeds=inp["negative_prompt_embeds"], negative_prompt_embeds=inp["prompt_embeds"])


# ------------------------------------------------------------------------------------------------------------------------------------
# blocks and pipeline
# ------------------------------------------------------------------------------------------------------------------------------------
def geglu_halves_swapped(nets, inp):
    """GEGLU's halves the other way round (gelu on the value half): the fused epilogue pairing column j with j + N/2 in the wrong order."""
    def forward(self, x):
        gate, h = self.proj(x).chunk(2, dim=-1)
        return h * torch.nn.functional.gelu(gate)
    return _attr(L.GEGLU, "forward", forward)


def pose_masked_swapped(nets, inp):
    """The 13 input channels assembled as [latents, mask, pose, masked image] instead of [latents, mask, masked image, pose]."""
    o_t = nets[0]
    orig = o_t.forward
    order = torch.tensor([0, 1, 2, 3, 4, 9, 10, 11, 12, 5, 6, 7, 8])
    return _attr(o_t, "forward", lambda sample, *a, **kw: orig(sample.index_select(1, order), *a, **kw))


def guidance_halves_swapped(nets, inp):
    """Classifier-free guidance with its halves exchanged: et + g (eu - et) instead of eu + g (et - eu)."""
    orig = opipe.denoise

    def denoise(unet, *a, **kw):
        def swapped(*ua, **ukw):
            eps = unet(*ua, **ukw)[0]
            b = eps.shape[0] // 2
            return (torch.cat([eps[b:], eps[:b]]),)
        return orig(swapped, *a, **kw)
    return _attr(opipe, "denoise", denoise)


def skip_order(nets, inp):
    """The skip stack popped in the wrong order: in every up block, the first two neighbouring skip tensors of equal shape exchanged."""
    def swapped(res):
        res = list(res)
        for i in range(len(res) - 1, 0, -1):                       # popped from the end
            if res[i].shape == res[i - 1].shape:
                res[i], res[i - 1] = res[i - 1], res[i]
                break
        return tuple(res)

    @contextlib.contextmanager
    def both():
        o1, o2 = U.CrossAttnUpBlock2D.forward, U.UpBlock2D.forward
        with _attr(U.CrossAttnUpBlock2D, "forward", lambda self, x, res, *a, **kw: o1(self, x, swapped(res), *a, **kw)), \
                _attr(U.UpBlock2D, "forward", lambda self, x, res, *a, **kw: o2(self, x, swapped(res), *a, **kw)):
            yield
    return both()


MUTANTS = {f.__name__: f for f in (
    log2e_scale, uniform, v_key_order_only, unmasked_pad_keys,
    garment_next_block, uncond_sees_garment, garment_tail_dropped, garments_swapped,
    cloth_text_ignored, timestep_stale,
    ip_scale_zero, ip_split_at_4, ip_rows_swapped, prompt_negative_swapped,
    geglu_halves_swapped, pose_masked_swapped, guidance_halves_swapped, skip_order)}
# defects that exist only at sizes whose token counts are no multiple of 16 (a no-op at 128x128)
SIZE_MUTANTS = {f.__name__: f for f in (unmasked_self_filler,)}


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference-only estimate of what 16-bit storage costs
# ------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def storage_rounded(nets, dtype):
    """Every leaf module of `nets` rounds its output to `dtype` and hands it on as fp32: the oracle's arithmetic with the engine's storage
    type between layers.  Measured against the clean oracle this is what a correct 16-bit engine may cost, without running one."""
    def hook(mod, args, out):
        return out.to(dtype).float() if torch.is_tensor(out) and out.is_floating_point() else out
    handles = [m.register_forward_hook(hook) for net in nets for m in net.modules() if not list(m.children())]
    try:
        yield
    finally:
        for h in handles:
            h.remove()
