"""What the guidance tests share: the issue's per-person values, the made-up argument struct of the refusal tests, the restatement of the
guided step in plain torch (any precision, on the CPU) that the kernel and the engine are compared against, the kernel's operands, and the
per-step replay of an engine call.  Importing this module needs no GPU and does not load the native library."""
import torch

G3, PHI3 = (7.5, 2.0, 1.0), (0.0, 0.7, 1.0)              # B = 3: no rescale at high guidance, both, full rescale at g = 1
COEF = (0.98, -0.03, 0.1)                                # c_x, c_eps, sigma of a mid-schedule DDPM step
HWS = (195, 4103)                                        # 15 x 13: below one block, with a tail; a prime: several waves and chunks per person
MARGIN = 4.0                                             # x the float32 evaluation's own error (the reduction order differs)


def guided_args(B=3, hw=195, ldc=64, branches=2, work_floats=None):
    """An idmvton_guided_step_args with made-up pointers: every call of the CPU tests is refused before a launch, none is dereferenced."""
    from idm_vton_amd import ffi
    a = ffi.GuidedStepArgs()
    a.dtype, a.B, a.hw, a.ldc, a.branches = ffi.BF16, B, hw, ldc, branches
    a.eps_nhwc, a.latents, a.noise, a.coef, a.work = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.work_floats = 8 * B * ((hw + 1023) // 1024) if work_floats is None else work_floats
    return a


def coef_row(g, phi, device="cpu", coef=COEF):
    return torch.tensor(list(coef) + list(g) + list(phi), dtype=torch.float32, device=device)


def formula(eps, lat, noise, coef, branches, dt):
    """The guided step of include/idmvton_hip.h restated in torch at precision `dt`, on the CPU, from the values as stored: eps NHWC
    [branches * B][hw][ldc] (16-bit; channels 0..3 read), lat / noise fp32 [B][4][hw] (noise may be None), coef the fp32 row
    {c_x, c_eps, sigma, g[B], phi[B]}.  e = u + g (t - u); where phi > 0 and branches == 2: e <- phi e std(t) / std(e) + (1 - phi) e with
    torch.std (unbiased) over the person's 4 hw elements; x = c_x x + c_eps e + sigma noise."""
    B = lat.shape[0]
    hw = lat.numel() // (4 * B)
    c = coef.detach().cpu().to(dt)
    e = eps.detach().cpu()[..., :4].to(dt).reshape(branches, B, hw, 4).permute(0, 1, 3, 2)
    g, phi = c[3:3 + B].view(B, 1, 1), c[3 + B:3 + 2 * B].view(B, 1, 1)
    if branches == 2:
        u, t = e[0], e[1]
        out = u + g * (t - u)
        for b in range(B):
            if float(phi[b]) > 0:
                out[b] = phi[b] * out[b] * (t[b].std() / out[b].std()) + (1 - phi[b]) * out[b]
    else:
        out = e[0]
    x = c[0] * lat.detach().cpu().to(dt).reshape(B, 4, hw) + c[1] * out
    if noise is not None:
        x = x + c[2] * noise.detach().cpu().to(dt).reshape(B, 4, hw)
    return x.reshape(lat.shape)


def errors(got, eps, lat, noise, coef, branches):
    """-> (the kernel's max-abs error against the fp64 formula / the formula's max-abs, the same for its float32 torch evaluation)."""
    ref = formula(eps, lat, noise, coef, branches, torch.float64)
    f32 = formula(eps, lat, noise, coef, branches, torch.float32)
    scale = ref.abs().max()
    return float((got.detach().cpu().double() - ref).abs().max() / scale), float((f32.double() - ref).abs().max() / scale)


def operands(B, hw, ldc, dtype, branches=2, seed=0):
    """-> (eps [branches * B][hw][ldc] with NaN in channels 4.., latents [B][4][hw], noise [B][4][hw]) on the CPU.  The two branches
    differ by a quarter of their scale and have a mean, as a model's predictions do, so the two standard deviations differ."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * hw + ldc + branches)
    t = torch.randn(B, hw, 4, generator=g) * 0.9 + 0.05
    rows = [t + 0.25 * torch.randn(B, hw, 4, generator=g), t] if branches == 2 else [t]
    eps = torch.full((branches * B, hw, ldc), float("nan"))
    eps[..., :4] = torch.cat(rows)
    return eps.to(dtype), torch.randn(B, 4, hw, generator=g), torch.randn(B, 4, hw, generator=g)


def emulate_cond_step(eps, lat, noise, coef):
    """The bits idmvton_guided_step(branches = 1) writes, from fp32 torch on the CPU: both products of c_x x + c_eps t rounded, then added
    (no FMA), and the noise term added with ONE rounding -- the fused multiply-add is formed in fp64, where the product of two fp32 values
    is exact (the sum is then rounded twice, to fp64 and to fp32: equal to one rounding unless the fp64 sum falls on an fp32 tie)."""
    B = lat.shape[0]
    hw = lat.numel() // (4 * B)
    c = coef.detach().cpu().float()
    t = eps.detach().cpu()[..., :4].float().reshape(B, hw, 4).permute(0, 2, 1)
    x = c[0] * lat.detach().cpu().float().reshape(B, 4, hw) + c[1] * t
    if noise is not None:
        x = (x.double() + c[2].double() * noise.detach().cpu().double().reshape(B, 4, hw)).float()
    return x.reshape(lat.shape)


def replay_eps(eng, st, i, latents):
    """Step i of a call on a device-resident 16-bit GarmentCache, from the given latents: pack_input + unet.forward with the launches the
    eager loop makes (tools/gpu_debug.py's one_step, on the cache's own views) -> eps.  Deterministic kernels: the loop's own bits."""
    from idm_vton_amd import ops
    B, branches = st["B"], st["branches"]
    st["latents"].copy_(latents)
    (ops.pack_input if branches == 2 else ops.pack_input_cond)(st["latents"], st["cond"], st["x_in"])
    eps, _ = eng.unet.forward(st["x_in"], st["temb_t"][i], st["ctx_t"], branches * B, st["h"], st["w"], garment_kv=st["gcache"].step(st["gidx"][i]),
                              garment_persons=st["garment_persons"], garment_hw=(st["gh"], st["gw"]), garment_index=st.get("gix"),
                              garment_nk=st.get("gnk"))
    return eps
