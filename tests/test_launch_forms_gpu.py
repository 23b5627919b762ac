"""-m gpu: the closure between the idmvton_gemm_conv launch forms the PRODUCT issues and the forms the kernel checks launch.

tests/launch_forms.py reduces a launch to everything that selects a code path (gather, activation, bias / residual / output types, colscale,
the V^T part, the epilogue width) and no sizes.  Here both sides are recorded through ops.RECORD:
  checked  one representative of every family of tests/kernel_checks.py::all_checks that reaches gemm_conv (fp16, the auto tile where the family
           has one): each of those is a comparison with a plain fp32 reference at the kernel's own bar;
  issued   the product's modules on the tiny configuration of tests/parity_utils.py, B = 2, serial eager, without any oracle: the engine at 128x128
           and at 264x200 (H*W % 16 != 0, short upsample grids), every constructor option that changes which launches are issued, the garment
           cache with projected K / V^T, the Resampler, both CLIP tower kinds and the boundary attention processors.
issued <= checked: a fused epilogue or a call site that lands without a kernel-level check fails here, naming the form field by field."""
import functools

import pytest
import torch

from tests import kernel_checks as kc
from tests.engine_support import clip_ids, clip_text, mk_attn
from tests.launch_forms import describe, gemm_form

pytestmark = pytest.mark.gpu
DT, DEV = torch.float16, "cuda"


class _Forms(list):
    """What ops.RECORD is set to: every GEMM record is reduced to its form at once, its keep-alive tensors are not kept."""

    def __init__(self):
        super().__init__()
        self.forms, self.launches = set(), 0

    def append(self, rec):
        if rec[0] == "gemm":
            self.forms.add(gemm_form(rec[2]))
            self.launches += 1


def record(fn):
    from idm_vton_amd import ops
    assert ops.RECORD is None
    rec = _Forms()
    ops.RECORD = rec
    try:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
    finally:
        ops.RECORD = None
    return rec


# ------------------------------------------------------------------------------------------------------------------ checked
NOT_GEMM = ("probe_", "attn_", "layernorm", "groupnorm", "elementwise", "quant_f8", "split_", "gn_precise", "softmax_", "layout_")
TAGS = sorted({t for _, t in kc.FORM_TILES} | {t for t, _ in kc.F8_OUT_TILES} | {"128x128", "128x64", "64x64", "128x256"}, key=len, reverse=True)


def family(name):
    """`ring_linear_K64_r128x64[f16]` -> (`ring_linear_K64`, `r128x64`); a name without a tile tag is its own family."""
    base = name[:name.rindex("[")]
    for t in TAGS:
        if base.endswith("_" + t):
            return base[:-len(t) - 1], t
    return base, ""


def representatives():
    """One fp16 (or split-precision) case per GEMM family: its auto-tile case where it has one, else the first listed."""
    reps = {}
    for name, fn, _ in kc.all_checks(DEV):
        if not (name.endswith("[f16]") or name.endswith("[split]")) or name.startswith(NOT_GEMM):
            continue
        fam, tag = family(name)
        if fam not in reps or (tag == "auto" and reps[fam][1] != "auto"):
            reps[fam] = (name, tag, fn)
    return reps


@functools.lru_cache(maxsize=None)
def _checked_by_family():
    """{family: (case name, its forms)}: every representative run once."""
    by = {}
    for fam, (name, _, fn) in representatives().items():
        rec = record(fn)
        assert rec.launches, f"{name}: listed as a GEMM family but launched none"
        by[fam] = (name, frozenset(rec.forms))
    return by


def checked(without=()):
    """-> {form: [case names]}.  without: families left out (the closure's own test below)."""
    forms = {}
    for fam, (name, fs) in _checked_by_family().items():
        if fam not in without:
            for f in fs:
                forms.setdefault(f, []).append(name)
    return forms


# ------------------------------------------------------------------------------------------------------------------ issued
@functools.lru_cache(maxsize=None)
def _model(**unet_kw):
    from tests import parity_utils as pu
    return pu.build("tiny", DT, DEV, unet_kw=unet_kw or None)


def _engine_call(H, W, steps=1, vae16=False, garment_cache=False, **unet_kw):
    from idm_vton_amd import config as pc
    from idm_vton_amd.pipeline import TryonEngine
    from idm_vton_amd.vae import HipVAE
    from tests import parity_utils as pu
    m = _model(**unet_kw)
    p_t, p_g, p_v, p_r = m["product"]
    if vae16:                                            # the 16-bit decoder instead of the split-precision one (same seeded weights as pu.build)
        vcfg = m["cfgs"][2]
        sd_v = {k: v.to(DT).float() for k, v in pc.random_state_dict(pc.vae_param_shapes(vcfg), 3, torch.float32, "cpu", std=0.05).items()}
        p_v = HipVAE(vcfg, sd_v, DT, DEV, precise_decode=False)
    eng = TryonEngine(p_t, p_g, p_v, p_r, DT, DEV)
    inp = pu.make_inputs(2, H, W, m["xd"], m["pooled"], m["enc_dim"], steps, DT)
    kw = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", **inp)

    def run():
        if garment_cache:
            cache = eng.encode_garment(num_inference_steps=steps, scheduler="ddpm", height=H, width=W, cloth=inp["cloth"],
                                       text_embeds_cloth=inp["text_embeds_cloth"], noise_cloth=inp["noise"]["cloth"])
            img = eng(**{**kw, "cloth": cache, "text_embeds_cloth": None, "noise": {**inp["noise"], "cloth": None}})
        else:
            img = eng(**kw)
        assert torch.isfinite(img).all()
    return run


def _clip(kind):
    def run():
        if kind == "text_quick_gelu":
            from idm_vton_amd.clip import HipCLIPText
            m = clip_text(128, 2, 2, "quick_gelu", 64, eos=2)
            HipCLIPText(m.state_dict(), m.config, DT, DEV)(clip_ids(3, 77, 1000, 999, 1))
        elif kind == "text_gelu":
            from idm_vton_amd.clip import HipCLIPText
            m = clip_text(128, 2, 2, "gelu", 64)
            HipCLIPText(m.state_dict(), m.config, DT, DEV)(clip_ids(3, 77, 1000, 999, 1))
        else:
            from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
            from idm_vton_amd.clip import HipCLIPVision
            torch.manual_seed(2)
            cfg = CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=224, patch_size=14,
                                   projection_dim=256, hidden_act="gelu")
            m = CLIPVisionModelWithProjection(cfg).eval()
            HipCLIPVision(m.state_dict(), m.config, DT, DEV)(torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)))
    return run


def _boundary():
    """The attention processors by the route of tests/test_boundary_gpu.py: self-attention on tokens (a multiple of 16 and not) and on NCHW, cross
    attention with 77 keys, text + image tokens."""
    from ip_adapter.attention_processor import AttnProcessor2_0, IPAttnProcessor2_0
    a = mk_attn(128, None, 2, AttnProcessor2_0(), 0)
    a(torch.randn(2, 100, 128).to(DEV, DT))
    a(torch.randn(2, 96, 128).to(DEV, DT))
    a(torch.randn(2, 128, 10, 10).to(DEV, DT))
    mk_attn(128, 192, 2, AttnProcessor2_0(), 1)(torch.randn(2, 72, 128).to(DEV, DT), encoder_hidden_states=torch.randn(2, 77, 192).to(DEV, DT))
    proc = IPAttnProcessor2_0(hidden_size=128, cross_attention_dim=192, scale=0.75, num_tokens=16)
    mk_attn(128, 192, 2, proc, 2)(torch.randn(2, 64, 128).to(DEV, DT), encoder_hidden_states=torch.randn(2, 93, 192).to(DEV, DT))


def _resampler():
    _model()["product"][3](torch.randn(2, 257, _model()["enc_dim"]).to(DT))


SOURCES = {
    "engine_128x128": lambda: _engine_call(128, 128, steps=2)(),
    "engine_264x200": lambda: _engine_call(264, 200)(),
    "engine_264x200_vae16": lambda: _engine_call(264, 200, vae16=True)(),
    "engine_128x128_vae16": lambda: _engine_call(128, 128, vae16=True)(),
    "engine_stream_f32_128x128": lambda: _engine_call(128, 128, stream_f32=True)(),
    "engine_stream_f32_264x200": lambda: _engine_call(264, 200, stream_f32=True)(),
    "engine_attn_fp8_128x128": lambda: _engine_call(128, 128, attn_fp8=True)(),
    "engine_attn_fp8_264x200": lambda: _engine_call(264, 200, attn_fp8=True)(),
    "engine_unfused_xattn_128x128": lambda: _engine_call(128, 128, fuse_xattn=False)(),
    "engine_garment_cache_128x128": lambda: _engine_call(128, 128, garment_cache=True)(),
    "resampler": _resampler,
    "clip_text_quick_gelu": lambda: _clip("text_quick_gelu")(),
    "clip_text_gelu": lambda: _clip("text_gelu")(),
    "clip_vision_gelu": lambda: _clip("vision")(),
    "boundary_attention_processors": _boundary,
}


@functools.lru_cache(maxsize=None)
def issued(source):
    rec = record(SOURCES[source])
    assert rec.launches, source
    return frozenset(rec.forms)


# ------------------------------------------------------------------------------------------------------------------ the closure
def _missing(forms, have):
    return "".join(f"\n  a form no kernel check launches:\n{describe(f)}" for f in sorted(forms - set(have), key=str))


@pytest.mark.parametrize("source", list(SOURCES))
def test_every_issued_form_has_a_kernel_check(source):
    have = checked()
    forms = issued(source)
    print(f"{source}: {len(forms)} form(s)")
    for f in sorted(forms, key=str):
        print("  ", tuple(f), "<-", have.get(f, ["NOT CHECKED"])[0])
    miss = _missing(forms, have)
    assert not miss, f"{source}:{miss}"


def test_recording_is_not_vacuous():
    """The issued set holds the forms this file exists for: an erf-GELU Linear, the row re-pitch, e4m3 output, GEGLU -- and the checked set is a
    set of forms, not of everything."""
    forms = set().union(*(issued(s) for s in SOURCES))
    print(f"{len(forms)} issued forms, {len(checked())} checked forms")
    for f in sorted(forms, key=str):
        print("  ", ", ".join(f"{k}={v}" for k, v in f._asdict().items()))
    assert any(f.mode == "GELU" for f in forms)
    assert any(f.mode == "QUICKGELU" for f in forms)
    assert any(f.gather == "rows_pad" for f in forms) and any(f.gather == "rows_crop" for f in forms)
    assert any(f.out == "e4m3" for f in forms) and any(f.vt != "none" and f.vt[2] for f in forms)
    assert any(f.mode == "GEGLU" for f in forms)
    assert any(f.mode == "XATTN" for f in forms) and any(f.ups == "short" for f in forms) and any(f.out == "f32" for f in forms)
    assert len(forms) >= 20


def test_a_dropped_check_is_named():
    """The closure's own test: without the row re-pitch family in the checked list, the engine at 264x200 must fail the closure with that form."""
    fams = tuple(sorted(f for f in representatives() if f.startswith("row_repitch")))
    assert fams
    gone = set(issued("engine_264x200")) - set(checked(without=fams))
    assert gone and all(f.gather in ("rows_pad", "rows_crop") for f in gone), gone
    assert "rows_pad" in _missing(issued("engine_264x200"), checked(without=fams))
