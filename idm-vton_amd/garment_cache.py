"""GarmentCache: the garment side of a try-on call, computed once and reused across calls and persons.

GarmentNet's inputs (cloth latent, cloth caption, timestep) never depend on the latents (pipeline.py's module docstring), so its 70
exported features -- and the attn1 K / V^T that TryonNet's to_k / to_v make of them -- are a pure function of (garment image, caption,
timestep, resolution, dtype mode, weights).  TryonEngine.encode_garment computes them for a timestep list; this class holds the result
and answers "which of my entries serve this call", refusing a call it was not built for before anything is launched.

Layout: per feature f one K tensor [n * G * N_f][C_f] and one V^T tensor [n * G][C_f][N_f] (16-bit, or e4m3 bytes where the fp8
self-attention takes its operands straight from the projection), timestep-major: timestep index i owns K rows [i * G * N_f, (i + 1) * G * N_f)
and V^T elements [i * G, (i + 1) * G).  A run of consecutive timesteps is therefore one contiguous slice of each tensor -- the shape of the
engine's persistent feature sets, so a block of timesteps moves into a set with one copy per tensor.  Plain torch, no kernels: usable on CPU
tensors (tests/test_garment_cache_cpu.py).

Two sizes: (h, w) is the PERSON latent size a cache is declared for -- what `check` holds a call to -- and (gh, gw) the garment's own latent
size, which fixes N_f (feature f has feature_tokens(gh, gw)[f] real tokens in round16 rows).  The K / V^T depend on the second alone, so
`for_person_size` re-declares a cache for another person size on the same tensors.  Size: with N1 / N2 the token rows at the two attention
levels of the SDXL topology (10 features of 640 channels, 60 of 1280), an entry is (10 * N1 * 640 + 60 * N2 * 1280) * 2 tensors * 2 bytes per
garment and timestep (tests/test_garment_size_cpu.py).
"""
import torch


def timestep_run(kv, n, G, i0, c=1):
    """THE layout rule, in one place: views of entries i0 .. i0 + c - 1 of a timestep-major (K, V^T) list that holds n timesteps of G
    elements -- K rows [i0 * r, (i0 + c) * r) with r = rows // n, V^T elements [i0 * G, (i0 + c) * G).  The cache itself, the engine's
    persistent sets and the rows encode_garment projects into are all cut with it."""
    out = []
    for k, vt in kv:
        r = k.shape[0] // n                              # K rows per timestep: G * N_f
        out.append((k[i0 * r:(i0 + c) * r], vt[i0 * G:(i0 + c) * G]))
    return out


def alloc_kv(shapes, n, m, device):
    """An uninitialised timestep-major (K, V^T) list for m timesteps, from the [(K shape, V^T shape, dtype)] of one that holds n."""
    return [(torch.empty((a[0] // n * m,) + tuple(a[1:]), dtype=d, device=device), torch.empty((b[0] // n * m,) + tuple(b[1:]), dtype=d, device=device))
            for a, b, d in shapes]


def kv_shapes(kv):
    return [(tuple(k.shape), tuple(vt.shape), k.dtype) for k, vt in kv]


class GarmentCache:
    def __init__(self, *, G, timesteps, h, w, dtype, attn_fp8, f8_exp, weights_id, kv, gh=None, gw=None):
        self.G = int(G)
        self.timesteps = [int(t) for t in timesteps]
        self.h, self.w = int(h), int(w)
        self.gh, self.gw = int(h if gh is None else gh), int(w if gw is None else gw)    # the garment's own latent size (default: the person's)
        self.dtype = dtype
        self.attn_fp8 = bool(attn_fp8)
        self.f8_exp = tuple(int(e) for e in f8_exp)
        self.weights_id = weights_id                     # TryonEngine.weights_identity(): GarmentNet's weights + TryonNet's attn1 to_k / to_v
        self.kv = list(kv)
        self._index = {t: i for i, t in enumerate(self.timesteps)}
        n = len(self.timesteps)
        if n < 1 or self.G < 1 or len(self._index) != n:
            raise ValueError(f"GarmentCache: needs G >= 1 and distinct timesteps (G={self.G}, timesteps={self.timesteps})")
        for f, (k, vt) in enumerate(self.kv):
            if k.shape[0] % (n * self.G) or vt.shape[0] != n * self.G or k.dtype != vt.dtype:
                raise ValueError(f"GarmentCache: feature {f} has K {tuple(k.shape)} / V^T {tuple(vt.shape)} for {n} timesteps x {self.G} garments")

    @property
    def nbytes(self):
        return sum(k.numel() * k.element_size() + vt.numel() * vt.element_size() for k, vt in self.kv)

    def __repr__(self):
        garment = f", garment latent={self.gh}x{self.gw}" if (self.gh, self.gw) != (self.h, self.w) else ""
        return (f"GarmentCache(G={self.G}, steps={len(self.timesteps)}, latent={self.h}x{self.w}{garment}, dtype={self.dtype}, "
                f"attn_fp8={self.attn_fp8}, {self.nbytes / 2 ** 20:.1f} MiB)")

    def _like(self, **kw):
        args = dict(G=self.G, timesteps=self.timesteps, h=self.h, w=self.w, gh=self.gh, gw=self.gw, dtype=self.dtype, attn_fp8=self.attn_fp8,
                    f8_exp=self.f8_exp, weights_id=self.weights_id, kv=self.kv)
        args.update(kw)
        return GarmentCache(**args)

    def for_person_size(self, h, w):
        """The same cache -- the same tensors, no copy -- declared for calls at person latent size (h, w).  The garment K / V^T are made from
        the cloth alone (GarmentNet at (gh, gw), TryonNet's attn1 to_k / to_v) and do not depend on the person's resolution, so one encoded
        garment serves e.g. 768x1024 and 1024x1536 calls; `check` stays strict, this is the explicit opt-in."""
        return self._like(h=h, w=w)

    def check(self, *, timesteps, h, w, dtype, attn_fp8, f8_exp, weights_id, persons):
        """The cache entry (timestep index) of every timestep of a call, looked up BY VALUE -- a cache built for n steps serves strength < 1
        (the last int(n * strength) of the same timesteps).  ValueError naming the field on any mismatch."""
        if (int(h), int(w)) != (self.h, self.w):
            raise ValueError(f"GarmentCache resolution mismatch: built for latent (h, w) = ({self.h}, {self.w}), the call runs at ({h}, {w})")
        if dtype != self.dtype:
            raise ValueError(f"GarmentCache dtype mismatch: built in {self.dtype}, the engine runs in {dtype}")
        if bool(attn_fp8) != self.attn_fp8:
            raise ValueError(f"GarmentCache attn_fp8 mismatch: built with attn_fp8={self.attn_fp8}, the engine has attn_fp8={bool(attn_fp8)}")
        if self.attn_fp8 and tuple(int(e) for e in f8_exp) != self.f8_exp:
            raise ValueError(f"GarmentCache f8_exp mismatch: built with exponents {self.f8_exp}, the engine uses {tuple(f8_exp)}")
        if weights_id != self.weights_id:
            raise ValueError(f"GarmentCache weights mismatch: built with weights {self.weights_id}, the engine holds {weights_id}")
        if persons < 1 or persons % self.G:
            raise ValueError(f"GarmentCache persons mismatch: P = {persons} persons is not a multiple of G = {self.G} garments "
                             "(conditional row i reads garment i % G)")
        missing = [int(t) for t in timesteps if int(t) not in self._index]
        if missing:
            raise ValueError(f"GarmentCache timesteps mismatch: {missing} are not among the {len(self.timesteps)} cached timesteps "
                             f"{self.timesteps[:3]}..{self.timesteps[-1:]} (same scheduler and num_inference_steps as encode_garment?)")
        return [self._index[int(t)] for t in timesteps]

    def run(self, i0, c=1):
        """Views of the 70 (K, V^T) pairs of cache entries i0 .. i0 + c - 1 (what TryonNet's attn1 reads as its garment segment)."""
        n, G = len(self.timesteps), self.G
        if not 0 <= i0 <= i0 + c <= n:
            raise IndexError(f"GarmentCache entries [{i0}, {i0 + c}) of {n}")
        return timestep_run(self.kv, n, G, i0, c)

    def step(self, i):
        return self.run(i, 1)

    def repeat_garments(self, times):
        """The same cache with every garment materialised `times` times (garment order g0..gG-1, g0..gG-1, ...): what a shared segment replaces.
        For tests and A/B measurements."""
        n, G = len(self.timesteps), self.G
        kv = []
        for k, vt in self.kv:
            r = k.shape[0] // n
            kk = k.reshape(n, 1, r, k.shape[1]).expand(n, times, r, k.shape[1]).reshape(n * times * r, k.shape[1]).contiguous()
            vv = vt.reshape(n, 1, G, *vt.shape[1:]).expand(n, times, G, *vt.shape[1:]).reshape(n * times * G, *vt.shape[1:]).contiguous()
            kv.append((kk, vv))
        return self._like(G=G * times, kv=kv)


def weights_fingerprint(named_tensors):
    """Identity of a weight set: a hash over (name, shape, dtype, fp64 sum, fp64 sum of |x|) of every tensor, in name order.  Two loads of one
    checkpoint in one storage dtype agree; another checkpoint, another dtype or one changed tensor does not (to the resolution of the two
    sums -- an identity check against mixing models up, not a cryptographic digest).  One device->host transfer for the whole set."""
    import hashlib
    names = sorted(named_tensors)
    if not names:
        return "empty"
    sums = torch.stack([torch.stack([named_tensors[k].double().sum(), named_tensors[k].double().abs().sum()]) for k in names]).cpu()
    hsh = hashlib.blake2b(digest_size=12)
    for k, s in zip(names, sums.tolist()):
        t = named_tensors[k]
        hsh.update(repr((k, tuple(t.shape), str(t.dtype), s[0], s[1])).encode())
    return hsh.hexdigest()
