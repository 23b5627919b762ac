"""DDPM (reference default: inference.py:232) and DDIM eta=0 (benchmark metric wording) step coefficients.

Host-side mirror of diffusers' DDPMScheduler.set_timesteps/step as the reference drives it (src/tryon_pipeline.py:1561,
1823) with the SDXL scheduler_config values (A.1): 1000 train steps, scaled_linear betas 0.00085..0.012,
timestep_spacing="leading", steps_offset=1, epsilon prediction, fixed_small variance, no clipping.  The update itself
runs on the GPU (idmvton_cfg_step): x_prev = c_x*x + c_eps*eps + sigma*noise; this file only produces the scalars.
"""
import numpy as np


class StepScheduler:
    def __init__(self, kind="ddpm", num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 set_alpha_to_one=False):
        if kind not in ("ddpm", "ddim"):
            raise ValueError(f"unknown scheduler kind {kind!r}")
        self.kind, self.T, self.steps_offset = kind, num_train_timesteps, steps_offset
        import torch                      # same float32 linspace / cumprod ops as diffusers' DDPMScheduler.__init__
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).double().numpy()
        # diffusers DDIMScheduler.final_alpha_cumprod: alphas_cumprod[0] unless set_alpha_to_one (SDXL scheduler_config: false);
        # used for the step whose previous timestep is < 0 (leading spacing + steps_offset=1: the LAST step, t = 1).
        # DDPMScheduler has no such switch: its previous alpha-bar is 1 there.
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.alphas_cumprod[0])
        self.init_noise_sigma = 1.0
        self.order = 1

    def set_timesteps(self, n):
        self.n = n
        ratio = self.T // n
        self.timesteps = (np.arange(0, n) * ratio).round()[::-1].astype(np.int64) + self.steps_offset
        return self.timesteps

    def coeffs(self, t):
        """(c_x, c_eps, sigma) of x_prev = c_x*x + c_eps*eps + sigma*noise for timestep t."""
        t = int(t)
        prev_t = t - self.T // self.n
        ab_t = float(self.alphas_cumprod[t])
        ab_p = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else (1.0 if self.kind == "ddpm" else self.final_alpha_cumprod)
        bb_t, bb_p = 1.0 - ab_t, 1.0 - ab_p
        if self.kind == "ddpm":
            a_t = ab_t / ab_p
            b_t = 1.0 - a_t
            c_x0 = (ab_p ** 0.5) * b_t / bb_t
            c_xt = (a_t ** 0.5) * bb_p / bb_t
            sigma = max(bb_p / bb_t * b_t, 1e-20) ** 0.5 if t > 0 else 0.0
            return c_xt + c_x0 / ab_t ** 0.5, -c_x0 * (bb_t ** 0.5) / ab_t ** 0.5, sigma
        return (ab_p ** 0.5) / ab_t ** 0.5, bb_p ** 0.5 - (ab_p ** 0.5) * (bb_t ** 0.5) / ab_t ** 0.5, 0.0

    def coef_table(self, timesteps, guidance_scale):
        """[steps][4] rows {c_x, c_eps, sigma, g}: what idmvton_cfg_step reads, one guidance for the whole batch."""
        return [list(self.coeffs(t)) + [float(guidance_scale)] for t in timesteps]

    def guided_coef_table(self, timesteps, guidance_scales, guidance_rescales):
        """[steps][3 + 2B] rows {c_x, c_eps, sigma, g[0..B), phi[0..B)}: what idmvton_guided_step reads -- a guidance scale and a
        guidance_rescale per person, the same in every step."""
        g, phi = [float(x) for x in guidance_scales], [float(x) for x in guidance_rescales]
        if len(g) != len(phi) or not g:
            raise ValueError(f"guided_coef_table: {len(g)} guidance scales and {len(phi)} rescales (one of each per person)")
        return [list(self.coeffs(t)) + g + phi for t in timesteps]

    def person_coef_table(self, timesteps, guidance_scales, guidance_rescales, n_active):
        """[steps][3 + 3B] rows {c_x, c_eps, sigma, g[0..B), phi[0..B), active[0..B)}: what idmvton_person_step reads -- the guided row plus,
        per person, whether it takes this step.  n_active[b] in [1, len(timesteps)] is person b's own step count (its strength): it is
        dormant (0.0) in the first len(timesteps) - n_active[b] loop steps and active (1.0) from then on, so its steps are the LAST
        n_active[b] timesteps -- what a call at its strength alone runs."""
        n, n_active = len(timesteps), [int(x) for x in n_active]
        rows = self.guided_coef_table(timesteps, guidance_scales, guidance_rescales)
        if len(n_active) != len(guidance_scales):
            raise ValueError(f"person_coef_table: {len(n_active)} step counts for {len(guidance_scales)} persons (one per person)")
        if any(not 1 <= x <= n for x in n_active):
            raise ValueError(f"person_coef_table: step counts {n_active} for a loop of {n} steps (each in [1, {n}])")
        return [row + [1.0 if i >= n - x else 0.0 for x in n_active] for i, row in enumerate(rows)]


def per_person(value, B, name):
    """A float or a sequence of B floats -> (list of B floats, whether a sequence was given).  ValueError naming the argument for a sequence
    of another length or a value that is no number."""
    if getattr(value, "ndim", None) == 0:                # a 0-d array / tensor is a scalar
        value = float(value)
    seq = hasattr(value, "__len__") or hasattr(value, "__iter__")
    vals = [v for v in value] if seq else [value] * B
    if seq and getattr(value, "ndim", 1) != 1:
        raise ValueError(f"`{name}` takes a float or a sequence of {B} floats, got shape {tuple(value.shape)}")
    if len(vals) != B:
        raise ValueError(f"`{name}` has {len(vals)} values for {B} persons: pass a float or one value per person")
    try:
        vals = [float(v) for v in vals]
    except (TypeError, ValueError):
        raise ValueError(f"`{name}` takes a float or a sequence of {B} floats, got {value!r}") from None
    if any(v != v for v in vals):
        raise ValueError(f"`{name}` holds NaN")
    return vals, seq
