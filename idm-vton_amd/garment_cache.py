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
`for_person_size` re-declares a cache for another person size on the same tensors.

A cache is also a POOL: with `garment_index` a call's person i wears garment garment_index[i] of the G (any P >= 1, values may repeat; the
attention kernels read the slot from a device table), and `select` / `cat` / `put` / `to` / `save` / `load` are what a resident pool is built
from -- `put` swaps one garment of a cache in place, so tensors, pointers and the engine's graph states stay valid.  GarmentPool keeps an LRU map
key -> slot over one such cache.  Size: with N1 / N2 the token rows at the two attention
levels of the SDXL topology (10 features of 640 channels, 60 of 1280), an entry is (10 * N1 * 640 + 60 * N2 * 1280) * 2 tensors * 2 bytes per
garment and timestep (tests/test_garment_size_cpu.py).

Mixed sizes: a cache that carries `sizes` -- one (gh, gw) per garment -- is SLOTTED: (gh, gw) is then the size its slots are laid out for, and
the garment of slot g, of latent size sizes[g], fills the front of the slot: K rows [0, N'_f) and V^T positions [0, ld'_f) of every feature and
timestep, with the rest of the V^T zero.  The attention kernels read each person's key count from a device table (the _ragged entry points),
so persons of one call wear garments of different sizes and a person with a small garment walks only its own key tiles.  Slots are always
16-bit: `put` widens an e4m3 feature (exactly: e4m3 times a power of two is a 16-bit number) and the fp8 attention quantises a slot per launch,
which gives the projection's own bytes back.  `take` returns a garment at its own compact size.  A cache without `sizes` is what it always was.

Packed storage: `pack()` gives a PackedGarmentCache -- the same tensors in the same layout as OCP e4m3 bytes (torch.uint8) plus one int32
exponent per (garment, feature, K | V^T) in `exps` [G][F][2]: half the resident bytes.  pack_exponent / pack_values / unpack_values below ARE the
format; the engine widens a block of timesteps into its 16-bit sets with one idmvton_kv_unpack launch, which matches them bit for bit.  Lossy
and opt-in, for the garment segment alone; `dtype` stays the engine's 16-bit dtype and every primitive moves `exps` with the bytes.

Host-resident: a cache whose tensors are CPU tensors (`to("cpu", pin_memory=True)`, GarmentPool(resident="host")) has `host_resident` true.
The engine takes one that is PAGE-LOCKED as `cloth=`: every block of timesteps then goes from host memory straight into the 16-bit sets by
one idmvton_kv_stream launch (pipeline.py, _cached_fill), so a catalogue is bounded by host RAM, not HBM.  Queued calls read such a cache
by raw address, with no stream order to protect them: a `put` into it waits for the device first and copies blocking.  With
host_transport="copy" the blocks cross the link by the copy engines into a staging arena instead and one idmvton_kv_place launch places them
(staged_plan below: the arena, the copy list and the place tables, for plain and shelved caches alike).

Features: a FEATURE cache (`features` true; encode_garment(storage="features")) holds what K and V^T are both made of -- per feature ONE
tensor F [n * G * N_f][C_f], GarmentNet's exported feature, pad rows included, in the engine's 16-bit dtype -- as one-tensor entries (F,) of
`kv`, under the same row rule: timestep_run cuts every tensor of an entry by its own rows per timestep.  Exactly half the bytes of the K / V^T
cache, with no loss; packed, `exps` is [G][F][1].  Every primitive here iterates the tensors of an entry and so serves both kinds; mixing
kinds is a ValueError naming `features`, and a feature cache's tensor list has no `sizes` (feature caches of several sizes live on a
shelf, below).  The engine projects each block of a call (pipeline.py, _cached_fill); TryonEngine.project_garment gives the K / V^T cache.

Shelf: a GarmentShelf is a host catalogue of garments of MANY sizes, each kept COMPACT -- a G = 1 cache of its own (N'_f rows, ld'_f V^T
positions) in page-locked memory, 16-bit or e4m3-packed -- so host RAM and the bytes a call moves over the host link follow the garments' own
sizes, not the largest one's.  `get` hands out a ShelvedGarmentCache: the garments of a batch as `parts`, declared for one slot size; the
engine puts each into the front of a slot of its 16-bit sets and writes the zero V^T tail behind it with one idmvton_kv_fill launch per block
(kv_records below, pipeline.py _cached_fill), and reads them as it reads a slotted cache.  A shelf of storage "features" / "features-e4m3"
holds compact FEATURE caches instead (half / a quarter of the bytes): the same launch puts each F into the front of a slot of a feature
staging list and writes the zero ROWS behind it, and the block's one projection makes the slot's K / V^T of them -- zero rows give the zero
V^T tail.  Sets, tables and graph states are those of the K / V^T shelf call at the same slot size.
"""
import torch


def timestep_run(kv, n, G, i0, c=1):
    """THE layout rule, in one place: views of entries i0 .. i0 + c - 1 of a timestep-major (K, V^T) list that holds n timesteps of G
    elements -- K rows [i0 * r, (i0 + c) * r) with r = rows // n, V^T elements [i0 * G, (i0 + c) * G).  The cache itself, the engine's
    persistent sets and the rows encode_garment projects into are all cut with it."""
    return [tuple(t[i0 * (t.shape[0] // n):(i0 + c) * (t.shape[0] // n)] for t in e) for e in kv]   # per timestep: G * N_f K rows, G V^T elements


def slot_run(kv, n, G, i, g0, c=1):
    """Views of garments g0 .. g0 + c - 1 of timestep entry i: timestep_run applied twice -- inside one timestep's views the G garments are
    laid out as that rule lays out timesteps of one element each."""
    return timestep_run(timestep_run(kv, n, G, i), G, 1, g0, c)


def index_runs(ids):
    """[3, 4, 5, 0, 1] -> [(0, 3, 3), (3, 0, 2)]: (destination slot, first source garment, count) of every run of consecutive garments."""
    runs = []
    for j, g in enumerate(ids):
        if runs and runs[-1][1] + runs[-1][2] == g:
            runs[-1] = (runs[-1][0], runs[-1][1], runs[-1][2] + 1)
        else:
            runs.append((j, g, 1))
    return runs


def alloc_kv(shapes, n, m, device):
    """An uninitialised timestep-major (K, V^T) list for m timesteps, from the [(K shape, V^T shape, dtype)] of one that holds n (a feature
    cache's list: [(F shape, dtype)])."""
    return [tuple(torch.empty((a[0] // n * m,) + tuple(a[1:]), dtype=e[-1], device=device) for a in e[:-1]) for e in shapes]


def kv_shapes(kv):
    return [tuple(tuple(t.shape) for t in e) + (e[0].dtype,) for e in kv]


def _f8_positions(ld):
    """position -> position: where the 16-bit kernels' key-ordered V^T keeps the key that the fp8 kernel's slot-ordered V^T holds at each of
    its ld positions (the inverse of idmvton_quant_f8 mode 1: position 64t + 32u + 16kb + 4g + j holds key 64t + 32kb + 8g + 4u + j, and the
    16-bit order swaps bits 2 and 3 of the key)."""
    pos = torch.arange(ld)
    key = (pos & ~63) | (((pos >> 4) & 1) << 5) | (((pos >> 2) & 3) << 3) | (((pos >> 5) & 1) << 2) | (pos & 3)
    return (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1)


def widen_f8(k8, vt8, dtype, ek, ev):
    """(K, V^T) of one feature as e4m3 bytes (the fp8 engine's fused projection: e4m3(x * 2^e), V^T in the fp8 kernel's slot order) -> the
    16-bit pair that idmvton_quant_f8 turns back into those bytes: e4m3 has 4 significant bits and |e| is small, so x' = e4m3 * 2^-e is
    exact in fp16 / bf16, and x' * 2^e rounds to the byte it came from."""
    k = (k8.view(torch.float8_e4m3fn).to(torch.float32) * 2.0 ** -ek).to(dtype)
    v = (vt8.view(torch.float8_e4m3fn).to(torch.float32) * 2.0 ** -ev).to(dtype)
    vt = torch.empty_like(v)
    vt[..., _f8_positions(v.shape[-1]).to(v.device)] = v
    return k, vt


# ---- the packed format ---------------------------------------------------------------------------------------------------
E4M3_MAX = 448.0
PACK_EXP_MIN, PACK_EXP_MAX = -7, 15


def pack_exponent(amax):
    """amax (a tensor of largest |x|, any float dtype) -> int32 e = clamp(floor(log2(448 / amax)), -7, 15), and 0 where amax is 0.  No
    division and no host sync: with amax = m * 2^x, m in [0.5, 1) (frexp), 448 / amax = (448 / m) * 2^-x and 448 / m lies in (448, 896], whose
    log2 has floor 9 when m <= 0.875 (448 / 0.875 = 512) and 8 otherwise.  The bounds: 448 * 2^7 < 65504 (x' fits fp16) and 2^-9 * 2^-15 is
    fp16's smallest subnormal (x' is exact in fp16 and bf16)."""
    m, x = torch.frexp(amax.float())
    e = torch.where(m <= 0.875, 9, 8) - x
    return torch.where(amax > 0, e.clamp(PACK_EXP_MIN, PACK_EXP_MAX), 0).to(torch.int32)


def _pow2(e):
    """int tensor e in [-126, 127] -> float32 2^e, built from the exponent bits (exact on every device)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def pack_values(x, e):
    """x (16-bit or float), e (int tensor broadcastable to x) -> uint8 OCP e4m3fn bytes of clamp(x * 2^e, +-448), round to nearest even.
    THE definition of the format, in plain torch (fp32 arithmetic: the product is exact)."""
    return (x.float() * _pow2(e)).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def unpack_values(b, e, dtype):
    """uint8 e4m3 bytes, e -> x' = e4m3(byte) * 2^-e in `dtype`: exact in fp16 and bf16 for e in [-7, 15]."""
    return (b.view(torch.float8_e4m3fn).float() * _pow2(-e)).to(dtype)


def _garment_major(t, n, G):
    """A timestep-major tensor [n * G * r][...] as [n][G][r * ...]: one garment's elements of every timestep along dims 0 and 2."""
    return t.reshape(n, G, -1)


class GarmentCache:
    packed = False                                       # PackedGarmentCache: True

    def __init__(self, *, G, timesteps, h, w, dtype, attn_fp8, f8_exp, weights_id, kv, gh=None, gw=None, sizes=None, rows=None, features=False):
        self.G = int(G)
        self.features = bool(features)                   # a FEATURE cache (module docstring): kv holds one-tensor entries (F,)
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
        # sizes: None, or the latent (gh, gw) of the garment in every slot of a slotted cache (module docstring); rows: per slot the (K rows,
        # V^T positions) per feature that garment fills -- what `take` cuts out -- or None for a slot that is filled to its end / never put
        self.sizes = None if sizes is None else [(int(a), int(b)) for a, b in sizes]
        self.rows = [None] * self.G if rows is None else [None if r is None else [(int(a), int(b)) for a, b in r] for r in rows]
        if self.sizes is not None and len(self.sizes) != self.G or len(self.rows) != self.G:
            raise ValueError(f"GarmentCache: sizes / rows need one entry per garment (G={self.G}, sizes={self.sizes})")
        if self.features:
            if (self.sizes is not None and self.kv) or self.attn_fp8:    # (sizes without a tensor list: a ShelvedGarmentCache of feature parts)
                raise ValueError("GarmentCache: features mismatch (a feature cache's tensor list has no `sizes` -- slotted caches hold K / V^T; "
                                 "features of several sizes live compact on a GarmentShelf -- and is not made or read by an attn_fp8 engine)")
            self.kv = [tuple(e) for e in self.kv]
            for f, e in enumerate(self.kv):
                if len(e) != 1 or e[0].dim() != 2 or e[0].shape[0] % (n * self.G):
                    raise ValueError(f"GarmentCache: feature {f} of a feature cache is one tensor F [n * G * N_f][C_f] for {n} timesteps x {self.G} "
                                     f"garments, got {[tuple(t.shape) for t in e]}")
            return
        for f, (k, vt) in enumerate(self.kv):
            if k.shape[0] % (n * self.G) or vt.shape[0] != n * self.G or k.dtype != vt.dtype:
                raise ValueError(f"GarmentCache: feature {f} has K {tuple(k.shape)} / V^T {tuple(vt.shape)} for {n} timesteps x {self.G} garments")

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for e in self.kv for t in e)

    @property
    def host_resident(self):
        """True when the tensors are CPU tensors (module docstring)."""
        return not self.kv[0][0].is_cuda

    def _put_mode(self):
        """-> nb(source): may a `put` copy from `source` be queued?  Into a device cache: yes from the device or from pinned memory (stream
        order protects queued calls).  Into a host-resident cache: never -- queued calls read it by raw address, so first everything queued
        on the device finishes, then the copies block ("copies to the host are complete on return")."""
        if not self.host_resident:
            return lambda s: s.is_cuda or s.is_pinned()
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        return lambda s: False

    def __repr__(self):
        garment = f", garment latent={self.gh}x{self.gw}" if (self.gh, self.gw) != (self.h, self.w) else ""
        if self.sizes is not None:
            garment = f", slots of {self.gh}x{self.gw} holding {sorted(set(self.sizes))}"
        return (f"GarmentCache(G={self.G}, steps={len(self.timesteps)}, latent={self.h}x{self.w}{garment}, dtype={self.dtype}, "
                f"attn_fp8={self.attn_fp8}, {'features, ' if self.features else ''}{self.nbytes / 2 ** 20:.1f} MiB)")

    def _args(self, **kw):
        args = dict(G=self.G, timesteps=self.timesteps, h=self.h, w=self.w, gh=self.gh, gw=self.gw, dtype=self.dtype, attn_fp8=self.attn_fp8,
                    f8_exp=self.f8_exp, weights_id=self.weights_id, kv=self.kv, sizes=self.sizes, rows=self.rows if self.sizes is not None else None,
                    features=self.features)
        args.update(kw)
        return args

    def _like(self, **kw):
        return GarmentCache(**self._args(**kw))

    def _carry(self, sources, device=None, pin_memory=False):
        """Constructor arguments beyond kv that a copy made of garments sources = [(cache, garment)] needs: none here (PackedGarmentCache: the
        exponents of those garments)."""
        return {}

    def for_person_size(self, h, w):
        """The same cache -- the same tensors, no copy -- declared for calls at person latent size (h, w).  The garment K / V^T are made from
        the cloth alone (GarmentNet at (gh, gw), TryonNet's attn1 to_k / to_v) and do not depend on the person's resolution, so one encoded
        garment serves e.g. 768x1024 and 1024x1536 calls; `check` stays strict, this is the explicit opt-in."""
        c = self._like(h=h, w=w)
        c.sizes, c.rows = self.sizes, self.rows          # shared like the tensors: a `put` through either is seen by both
        return c

    def check(self, *, timesteps, h, w, dtype, attn_fp8, f8_exp, weights_id, persons, garment_index=None):
        """The cache entry (timestep index) of every timestep of a call, looked up BY VALUE -- a cache built for n steps serves strength < 1
        (the last int(n * strength) of the same timesteps).  ValueError naming the field on any mismatch.
        garment_index (person i wears garment garment_index[i]): replaces the P % G rule by len == persons and 0 <= v < G, and the result is
        the pair (cache entries, garment_index as a validated list of ints) -- what the engine needs of an indexed call."""
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
        ids = None
        if garment_index is not None:
            ids = self.garment_ids(garment_index, persons)
        elif persons < 1 or persons % self.G:
            raise ValueError(f"GarmentCache persons mismatch: P = {persons} persons is not a multiple of G = {self.G} garments "
                             "(conditional row i reads garment i % G)")
        missing = [int(t) for t in timesteps if int(t) not in self._index]
        if missing:
            raise ValueError(f"GarmentCache timesteps mismatch: {missing} are not among the {len(self.timesteps)} cached timesteps "
                             f"{self.timesteps[:3]}..{self.timesteps[-1:]} (same scheduler and num_inference_steps as encode_garment?)")
        entries = [self._index[int(t)] for t in timesteps]
        return entries if ids is None else (entries, ids)

    def garment_ids(self, garment_index, persons):
        """garment_index as a list of `persons` ints in [0, G); ValueError naming the field otherwise."""
        try:
            ids = [int(v) for v in (garment_index.tolist() if isinstance(garment_index, torch.Tensor) else garment_index)]
        except (TypeError, ValueError):
            raise ValueError(f"GarmentCache garment_index mismatch: expected a sequence of {persons} ints, got {garment_index!r}") from None
        if persons < 1 or len(ids) != persons:
            raise ValueError(f"GarmentCache garment_index mismatch: {len(ids)} entries for P = {persons} persons (one garment per person)")
        bad = [v for v in ids if not 0 <= v < self.G]
        if bad:
            raise ValueError(f"GarmentCache garment_index mismatch: {bad} outside [0, G = {self.G}) garments")
        return ids

    def garment_sizes(self, garment_index, persons=None):
        """The latent (gh, gw) of the garment each person wears, for a garment_index that `garment_ids` accepts: sizes[garment_index[i]] on a
        slotted cache, the cache's one (gh, gw) otherwise."""
        ids = self.garment_ids(garment_index, len(garment_index) if persons is None else persons)
        return [self.sizes[g] if self.sizes is not None else (self.gh, self.gw) for g in ids]

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
        rep = lambda t: t.reshape(n, 1, -1).expand(n, times, t.numel() // n).reshape((t.shape[0] * times,) + t.shape[1:]).contiguous()
        kv = [tuple(rep(t) for t in e) for e in self.kv]
        return self._like(G=G * times, kv=kv, sizes=None if self.sizes is None else self.sizes * times, rows=self.rows * times,
                          **self._carry([(self, g) for _ in range(times) for g in range(G)]))


    # ---- the pool primitives --------------------------------------------------------------------------------------------
    _FIELDS = ("timesteps", "h", "w", "gh", "gw", "dtype", "attn_fp8", "f8_exp", "weights_id")

    def _agrees(self, other, what, devices=True):
        """ValueError naming the first field in which `other` differs from this cache (G aside; devices=False: and where its tensors live)."""
        if self.features != other.features:
            raise ValueError(f"GarmentCache {what}: features mismatch ({self.features} against {other.features}: a feature cache holds GarmentNet's "
                             "features, a K / V^T cache their projections -- engine.project_garment(features) gives the K / V^T cache)")
        if self.packed != other.packed:
            raise ValueError(f"GarmentCache {what}: packed mismatch ({self.packed} against {other.packed}: pack() or unpack() one of them)")
        for f in self._FIELDS:
            if getattr(self, f) != getattr(other, f):
                raise ValueError(f"GarmentCache {what}: {f} mismatch ({getattr(self, f)} against {getattr(other, f)})")
        n = len(self.timesteps)
        facts = lambda c: [(e[0].shape[0] // (n * c.G),) + tuple(x for t in e for x in t.shape[1:]) + (e[0].dtype, e[0].device.type if devices else None)
                           for e in c.kv]
        mine, theirs = facts(self), facts(other)
        if mine != theirs:
            raise ValueError(f"GarmentCache {what}: kv mismatch (feature shapes, dtypes or devices differ)")

    def _gather(self, sources):
        """A new cache (a copy) whose garment j is garment g of cache c for (c, g) = sources[j]."""
        n, U = len(self.timesteps), len(sources)
        kv = alloc_kv(kv_shapes(timestep_run(self.kv, n, self.G, 0)), self.G, n * U, self.kv[0][0].device)
        # consecutive garments of one source move as one run (index_runs, per stretch of one source)
        runs, j = [], 0
        while j < U:
            e = j
            while e < U and sources[e][0] is sources[j][0]:
                e += 1
            runs += [(j + d0, sources[j][0], g0, c) for d0, g0, c in index_runs([g for _, g in sources[j:e]])]
            j = e
        for i in range(n):
            for j0, src, g0, c in runs:
                for d, s in zip(slot_run(kv, n, U, i, j0, c), slot_run(src.kv, n, src.G, i, g0, c)):
                    for dt, st in zip(d, s):
                        dt.copy_(st)
        slotted = any(c.sizes is not None for c, _ in sources)       # equal slot size (_agrees): whole slots moved, the sizes go along
        return self._like(G=U, kv=kv, sizes=[c.sizes[g] if c.sizes is not None else (c.gh, c.gw) for c, g in sources] if slotted else None,
                          rows=[c.rows[g] for c, g in sources] if slotted else None, **self._carry(sources))

    def select(self, ids):
        """A new cache (a copy) of garments ids[0], ids[1], ... of this one, in that order; values may repeat."""
        ids = self.garment_ids(ids, len(ids))
        return self._gather([(self, g) for g in ids])

    @staticmethod
    def cat(caches):
        """One cache of sum(G) garments (a copy) from caches that agree in every other field; ValueError naming the field otherwise."""
        caches = list(caches)
        if not caches:
            raise ValueError("GarmentCache cat: no caches")
        for c in caches[1:]:
            caches[0]._agrees(c, "cat")
        return caches[0]._gather([(c, g) for c in caches for g in range(c.G)])

    def put(self, slot, other):
        """Overwrite garment `slot` IN PLACE with the one garment of `other` (G = 1, every other field equal): the tensors, their pointers and
        the engine's graph states stay valid -- how a resident pool swaps a garment.  `other` may live on another device (a garment spilled to
        the host comes back without a temporary device copy).  Stream-ordered copies: calls already queued read the old garment, later ones
        the new; only a pinned host source is copied asynchronously.  Into a HOST-RESIDENT cache: queued device work is waited for first and
        the copies block (_put_mode), so calls already queued read the old garment and the new one is complete on return."""
        if not 0 <= int(slot) < self.G:
            raise ValueError(f"GarmentCache put: slot mismatch ({slot} outside [0, G = {self.G}))")
        if other.G != 1:
            raise ValueError(f"GarmentCache put: G mismatch (takes a cache of one garment, got G = {other.G})")
        if self.sizes is not None:
            if other.features:
                raise ValueError("GarmentCache put: features mismatch (a cache with `sizes` (slotted / mixed_sizes) holds K / V^T: slots of features "
                                 "are not built -- engine.project_garment(features) gives the K / V^T garment)")
            return self._put_slotted(int(slot), other)
        self._agrees(other, "put", devices=False)
        n = len(self.timesteps)
        nb = self._put_mode()
        for i in range(n):
            for d, s in zip(slot_run(self.kv, n, self.G, i, int(slot)), timestep_run(other.kv, n, 1, i)):
                for dt, st in zip(d, s):
                    dt.copy_(st, non_blocking=nb(st))
        return self

    def _put_slotted(self, slot, other):
        """`put` on a cache with `sizes`: the garment of `other` may be of another (smaller) size than the slots.  Every feature's K rows and
        V^T positions must fit the slot's ("does not fit" otherwise, before any copy); they go to the front of the slot and the rest of the
        slot's V^T is zero-filled -- the fp8 attention quantises whole slots and permutes inside 64-key tiles, so a stale value next to the
        last real ones would meet a zero probability as NaN.  The K tail keeps what it held: no kernel reads a K row beyond a garment's count.
        An e4m3 feature of `other` is widened (widen_f8): slots are 16-bit."""
        for f in self._FIELDS:
            if f not in ("gh", "gw") and getattr(self, f) != getattr(other, f):
                raise ValueError(f"GarmentCache put: {f} mismatch ({getattr(self, f)} against {getattr(other, f)})")
        n = len(self.timesteps)
        size = other.sizes[0] if other.sizes is not None else (other.gh, other.gw)
        if len(self.kv) != len(other.kv):
            raise ValueError(f"GarmentCache put: does not fit ({len(other.kv)} features against {len(self.kv)})")
        fill = []                                        # per feature: (K rows, V^T positions) the garment fills
        for f, ((k, vt), (ok, ovt)) in enumerate(zip(self.kv, other.kv)):
            N, Nf = k.shape[0] // (n * self.G), ok.shape[0] // n
            if other.rows[0] is not None:
                Nf, ldf = other.rows[0][f]
            else:
                ldf = ovt.shape[2]
            ok_dtype = ok.dtype == k.dtype or (ok.dtype == torch.uint8 and self.attn_fp8 and k.dtype != torch.uint8)
            if k.shape[1:] != ok.shape[1:] or vt.shape[1] != ovt.shape[1] or Nf > N or ldf > vt.shape[2] or not ok_dtype:
                raise ValueError(f"GarmentCache put: does not fit (feature {f}: a garment of latent {size[0]}x{size[1]} has K rows {Nf} x {tuple(ok.shape[1:])} "
                                 f"{ok.dtype} and V^T {ovt.shape[1]} x {ldf}, a slot of {self.gh}x{self.gw} holds {N} x {tuple(k.shape[1:])} {k.dtype} and "
                                 f"{vt.shape[1]} x {vt.shape[2]})")
            fill.append((Nf, ldf))
        for i in range(n):
            for (Nf, ldf), (dk, dv), (sk, sv) in zip(fill, slot_run(self.kv, n, self.G, i, slot), timestep_run(other.kv, n, 1, i)):
                if sk.dtype != dk.dtype:
                    sk, sv = widen_f8(sk, sv, dk.dtype, self.f8_exp[1], self.f8_exp[2])
                nb = sk.is_cuda or sk.is_pinned()
                dk[:Nf].copy_(sk[:Nf], non_blocking=nb)
                dv[..., :ldf].copy_(sv[..., :ldf], non_blocking=nb)
                dv[..., ldf:].zero_()
        self.sizes[slot] = size
        self.rows[slot] = None if all(a == k.shape[0] // (n * self.G) and b == vt.shape[2] for (a, b), (k, vt) in zip(fill, self.kv)) else fill
        return self

    def take(self, slot, device=None, pin_memory=False):
        """A new G = 1 cache holding garment `slot` (a copy), on `device` (default: where the cache lives) -- copied slot view by slot view
        straight into the destination (pin_memory: page-locked host tensors), with no intermediate copy on the source device.  Copies to the
        host are complete when this returns."""
        if not 0 <= int(slot) < self.G:
            raise ValueError(f"GarmentCache take: slot mismatch ({slot} outside [0, G = {self.G}))")
        n = len(self.timesteps)
        device = self.kv[0][0].device if device is None else torch.device(device)
        pin = bool(pin_memory) and device.type == "cpu"
        if self.features:                                # one tensor per feature, never slotted: the slot's rows as they are
            kv = [(torch.empty((f.shape[0] // self.G, f.shape[1]), dtype=f.dtype, device=device, pin_memory=pin),) for f, in self.kv]
            for i in range(n):
                for (d,), (s,) in zip(timestep_run(kv, n, 1, i), slot_run(self.kv, n, self.G, i, int(slot))):
                    d.copy_(s)
            return self._like(G=1, kv=kv, **self._carry([(self, int(slot))], device, pin))
        # a slotted cache gives the garment back at its own compact size: the rows / positions `put` filled
        fill = self.rows[int(slot)] or [(k.shape[0] // (n * self.G), vt.shape[2]) for k, vt in self.kv]
        kv = [(torch.empty((n * Nf,) + tuple(k.shape[1:]), dtype=k.dtype, device=device, pin_memory=pin),
               torch.empty((n, vt.shape[1], ldf), dtype=vt.dtype, device=device, pin_memory=pin)) for (Nf, ldf), (k, vt) in zip(fill, self.kv)]
        for i in range(n):
            for (Nf, ldf), (dk, dv), (sk, sv) in zip(fill, timestep_run(kv, n, 1, i), slot_run(self.kv, n, self.G, i, int(slot))):
                dk.copy_(sk[:Nf])
                dv.copy_(sv[..., :ldf])
        if self.sizes is None:
            return self._like(G=1, kv=kv, **self._carry([(self, int(slot))], device, pin))
        return self._like(G=1, kv=kv, gh=self.sizes[int(slot)][0], gw=self.sizes[int(slot)][1], sizes=None, rows=None)

    def to(self, device, pin_memory=False):
        """The same cache on another device (host offload and return): one copy per tensor; pin_memory: page-locked host tensors, so that
        the way back is an asynchronous copy.  Copies TO the host are blocking -- the result is complete when this returns and may be read,
        compared or saved at once; only pinned host -> device is queued asynchronously (stream-ordered before any later launch).  The same
        device without pinning returns self."""
        device = torch.device(device)
        if not pin_memory and all(e[0].device == device for e in self.kv):
            return self

        def move(t):
            if pin_memory and device.type == "cpu":
                out = torch.empty(t.shape, dtype=t.dtype, device="cpu", pin_memory=True)
                out.copy_(t)
                return out
            return t.to(device, non_blocking=device.type != "cpu" and t.device.type == "cpu" and t.is_pinned())
        return self._like(kv=[tuple(move(t) for t in e) for e in self.kv])

    FORMAT_VERSION = 1

    def save(self, path):
        """-> a safetensors file: tensors k.<f> / vt.<f> (e4m3 caches are uint8 bytes) and a metadata record (format version, G, timesteps, both
        sizes, dtype, attn_fp8, f8_exp, weights_id).  A cache with `sizes` writes format version 2, which adds sizes and rows; one without
        writes version 1 exactly as before.  A packed cache writes version 3: `packed: true` and the tensor `exps`.  A FEATURE cache writes
        version 4: `kind: "features"`, tensors f.<f> in place of k / vt, and -- packed -- `packed: true` and `exps` as in version 3."""
        import json
        from safetensors.torch import save_file
        tensors = {}
        for f, e in enumerate(self.kv):
            for name, t in zip(("f",) if self.features else ("k", "vt"), e):
                tensors[f"{name}.{f:03d}"] = t.detach().cpu().contiguous()
        meta = dict(format="idmvton_garment_cache", version=self.FORMAT_VERSION, G=self.G, timesteps=self.timesteps, h=self.h, w=self.w, gh=self.gh,
                    gw=self.gw, dtype=str(self.dtype), attn_fp8=self.attn_fp8, f8_exp=list(self.f8_exp), weights_id=self.weights_id, features=len(self.kv))
        if self.packed:                                  # version 3: e4m3 bytes + the exponents
            meta.update(version=3, packed=True)
            tensors["exps"] = self.exps.detach().cpu().contiguous()
        if self.sizes is not None:
            meta.update(version=2, sizes=[list(sz) for sz in self.sizes], rows=[None if r is None else [list(x) for x in r] for r in self.rows])
        if self.features:
            meta.update(version=4, kind="features")
        save_file(tensors, path, metadata={k: json.dumps(v) for k, v in meta.items()})

    @staticmethod
    def load(path, device="cpu"):
        """The cache `save` wrote, on `device`.  What it was built for travels in the metadata, so `check` refuses it on any other engine with
        the messages it has for a cache made in this process."""
        import json
        from safetensors import safe_open
        with safe_open(path, framework="pt", device=str(device)) as f:
            meta = {k: json.loads(v) for k, v in (f.metadata() or {}).items()}
            if meta.get("format") != "idmvton_garment_cache" or meta.get("version") not in (GarmentCache.FORMAT_VERSION, 2, 3, 4):
                raise ValueError(f"GarmentCache load: {path} is not a garment cache of format version {GarmentCache.FORMAT_VERSION} "
                                 f"(format={meta.get('format')!r}, version={meta.get('version')!r})")
            feats = meta.get("kind") == "features"
            kv = [tuple(f.get_tensor(f"{name}.{i:03d}") for name in (("f",) if feats else ("k", "vt"))) for i in range(meta["features"])]
            exps = f.get_tensor("exps") if meta.get("packed") else None
        dtype = {str(d): d for d in (torch.float16, torch.bfloat16, torch.float32)}[meta["dtype"]]
        args = dict(G=meta["G"], timesteps=meta["timesteps"], h=meta["h"], w=meta["w"], gh=meta["gh"], gw=meta["gw"], dtype=dtype,
                    attn_fp8=meta["attn_fp8"], f8_exp=meta["f8_exp"], weights_id=meta["weights_id"], kv=kv, sizes=meta.get("sizes"), rows=meta.get("rows"), features=feats)
        return PackedGarmentCache(exps=exps, **args) if exps is not None else GarmentCache(**args)

    # ---- packed storage ---------------------------------------------------------------------------------------------------
    def pack_exps(self):
        """int32 [G][F][2] (0 = K, 1 = V^T; a feature cache: [G][F][1]): pack_exponent of the largest |x| of every garment's tensors over ALL
        timesteps, on the device the cache lives on, without a host sync."""
        n, G = len(self.timesteps), self.G
        amax = [torch.stack([_garment_major(t, n, G).abs().amax(dim=(0, 2)).float() for t in kvf], dim=-1) for kvf in self.kv]   # F x [G][2]
        return pack_exponent(torch.stack(amax, dim=1))

    def pack(self, exps=None):
        """-> PackedGarmentCache (a copy): every K / V^T as e4m3 bytes under one exponent per (garment, feature, tensor) -- half the bytes.
        Lossy: |x' - x| <= 2^-4 |x| where |x| * 2^e >= 2^-6, <= 2^-10 * 2^-e below.  On the GPU the bytes come from idmvton_quant_f8 (mode 0,
        bit-equal to the torch conversion) applied to x * 2^e.  ValueError for a cache with `sizes`, an attn_fp8 cache and a packed one."""
        if self.packed:
            raise ValueError("GarmentCache pack: the cache is already e4m3-packed")
        if self.sizes is not None:
            raise ValueError("GarmentCache pack: a cache with `sizes` (slotted / mixed_sizes) cannot be packed: its slots are 16-bit")
        if self.attn_fp8:
            raise ValueError("GarmentCache pack: an attn_fp8 cache cannot be packed: its features already are e4m3 operands of the fp8 attention")
        n, G = len(self.timesteps), self.G
        exps = self.pack_exps() if exps is None else exps
        kv = []
        for f, kvf in enumerate(self.kv):
            kv.append(tuple(_pack_tensor(t, exps[:, f, j], n, G) for j, t in enumerate(kvf)))
        return PackedGarmentCache(exps=exps, **self._args(kv=kv))


def _pack_tensor(t, e, n, G):
    """One timestep-major K / V^T tensor under its garments' exponents e [G] -> bytes of the same shape."""
    if not t.is_cuda:
        return pack_values(_garment_major(t, n, G), e.view(1, G, 1)).reshape(t.shape)
    from . import ops                                    # the HIP conversion; x * 2^e in the 16-bit dtype is exact where the byte is not 0
    scaled = (_garment_major(t, n, G) * _pow2(e).view(1, G, 1)).to(t.dtype).reshape(-1, t.shape[-1])
    return ops.quant_f8(scaled, 1.0).reshape(t.shape)


class PackedGarmentCache(GarmentCache):
    """A GarmentCache whose K / V^T are e4m3 bytes (module docstring): kv tensors are torch.uint8 in the 16-bit layout, `exps` int32 [G][F][2]
    on the same device.  `dtype` is the 16-bit dtype the engine widens into, attn_fp8 is False, `sizes` is None."""
    packed = True

    def __init__(self, *, exps=None, **kw):
        super().__init__(**kw)
        if self.sizes is not None or self.attn_fp8 or any(e[0].dtype != torch.uint8 for e in self.kv):
            raise ValueError("PackedGarmentCache: holds e4m3 bytes (torch.uint8) of a cache without `sizes` and without attn_fp8")
        dev = self.kv[0][0].device
        T = len(self.kv[0])                              # tensors per feature: (K, V^T), or the one F of a feature cache
        self.exps = torch.zeros(self.G, len(self.kv), T, dtype=torch.int32, device=dev) if exps is None else exps
        if tuple(self.exps.shape) != (self.G, len(self.kv), T) or self.exps.dtype != torch.int32 or self.exps.device.type != dev.type:
            raise ValueError(f"PackedGarmentCache: exps must be int32 [G = {self.G}][F = {len(self.kv)}][{T}] on {dev.type}, got "
                             f"{self.exps.dtype} {tuple(self.exps.shape)} on {self.exps.device.type}")

    @property
    def nbytes(self):
        return GarmentCache.nbytes.fget(self) + self.exps.numel() * self.exps.element_size()

    def __repr__(self):
        return "Packed" + super().__repr__()[:-1] + ", e4m3-packed)"

    def _like(self, **kw):
        """exps go with the tensors: shared when the tensors are (for_person_size), else the caller's (`_carry`) or zeros -- a pool's empty slots."""
        args = self._args(**kw)
        if "exps" not in kw and "kv" not in kw:
            args["exps"] = self.exps
        return PackedGarmentCache(**args)

    def _carry(self, sources, device=None, pin_memory=False):
        dev = self.exps.device if device is None else torch.device(device)
        out = torch.empty((len(sources),) + tuple(self.exps.shape[1:]), dtype=torch.int32, device=dev, pin_memory=bool(pin_memory) and dev.type == "cpu")
        for j, (c, g) in enumerate(sources):
            out[j].copy_(c.exps[g])
        return dict(exps=out)

    def for_person_size(self, h, w):
        return self._like(h=h, w=w)                      # the same tensors and the same exps

    def put(self, slot, other):
        """As GarmentCache.put, for a packed G = 1 cache (bytes and exponents copied in place) or a 16-bit one, which is packed first on the
        device it lives on.  The exponents travel on the same stream as the bytes: calls already queued read the old garment whole."""
        if not other.packed and other.G == 1 and 0 <= int(slot) < self.G:
            other = other.pack()
        super().put(slot, other)
        src = other.exps[0]
        self.exps[int(slot)].copy_(src, non_blocking=not self.host_resident and (src.is_cuda or src.is_pinned()))
        return self

    def to(self, device, pin_memory=False):
        c = super().to(device, pin_memory)
        if c is not self:
            device = torch.device(device)
            if pin_memory and device.type == "cpu":
                c.exps = torch.empty(self.exps.shape, dtype=torch.int32, device="cpu", pin_memory=True)
                c.exps.copy_(self.exps)
            else:
                c.exps = self.exps.to(device, non_blocking=device.type != "cpu" and self.exps.device.type == "cpu" and self.exps.is_pinned())
        return c

    def unpack(self):
        """-> the 16-bit GarmentCache (a copy) of x' = e4m3(byte) * 2^-e: exactly what the engine's sets hold during a call on this cache (on
        the GPU the same idmvton_kv_unpack kernel writes it)."""
        n, G = len(self.timesteps), self.G
        kv = alloc_kv([e[:-1] + (self.dtype,) for e in kv_shapes(self.kv)], n, n, self.kv[0][0].device)
        if self.kv[0][0].is_cuda:
            from . import ops
            ops.KvUnpackTable(fill_records(self.kv, n, G, kv, n, G, self.exps, list(range(n)), list(range(n)), list(range(G)), list(range(G))),
                              self.kv[0][0].device).launch(self.dtype)
        else:
            for f, (src, dst) in enumerate(zip(self.kv, kv)):
                for j in range(len(src)):
                    _garment_major(dst[j], n, G).copy_(unpack_values(_garment_major(src[j], n, G), self.exps[:, f, j].view(1, G, 1), self.dtype))
        return GarmentCache(**self._args(kv=kv))


def kv_records(sources, dst_kvs, k, S, entries, tslots, address=None):
    """THE descriptor records (int64 [N][5]: ops.KvUnpackTable and the idmvton_kv_stream / _fill / _place tables) that move garments into each
    of the 16-bit lists dst_kvs (the sets: k timesteps of S garment slots, of equal shapes), for every pair (entry i, timestep slot j) of
    (entries, tslots): first all records of dst_kvs[0], then those of dst_kvs[1], ...  A SOURCE is
    (kv, n, G, garments, gslots, exps): garment g of the timestep-major list kv (n timesteps of G) goes into garment slot u, for every pair
    (g, u) of (garments, gslots) -- some garments of a cache, one shelf part (G = 1, garment 0) or their image in a staging arena.  Pure
    address arithmetic on the one layout rule (timestep_run / slot_run): (i, g) of a tensor starts (i * G + g) * (elements per garment and
    timestep) after its base, so per feature a garment is a base address, G such units to advance per entry, and its own N'_f K rows and
    ld'_f V^T positions, which may be fewer than the slot's N_f / ld_f.  Per (timestep, source, garment, feature), in that order:
      K      one data run of the N'_f rows into the front of the slot (rows beyond are not written: no kernel reads them);
      V^T    one data run of C_f rows x ld'_f positions, source row stride ld'_f, destination row stride ld_f;
      tail   exactly where ld'_f < ld_f, one ZERO RUN (src 0) of C_f rows x (ld_f - ld'_f) positions behind it -- the whole tail, as _put_slotted
             writes it, so a set's V^T depends on the garment alone and not on what the slot held before.
    FEATURE lists (one-tensor entries (F,), source and destination alike: a staging list that project_garment_kv reads) have, per (timestep,
    source, garment, feature):
      F      one data run of the N'_f rows into the front of the slot;
      rows   exactly where N'_f < N_f, one ZERO RUN (src 0, exp 0) of (N_f - N'_f) rows x C_f directly behind it -- the whole row tail: the
             projection reads every row of a slot, and zero rows project to the zero K rows and the zero V^T tail (to_k / to_v have no bias).
    exps (int32 [G][F][2]; feature lists: [G][F][1]) gives the WIDENING form: the source is e4m3 bytes, cols / lds in bytes = elements,
    ldd in 16-bit elements, exp the address of the garment's exponent.  exps None gives the COPY form: a 16-bit source, cols, lds and ldd in BYTES, exp 0.  An odd number of
    records per timestep is made even by repeating the smallest (a slice of a table starts at an even index; identical bytes written twice
    are what clamped lanes already do).  address(tensor) -> the address a kernel reads the tensor's first element under (default
    data_ptr(); ops.stream_address for a host-resident source); it is asked once per source tensor.
    -> (records, per): timestep number t of (entries, tslots) owns records [t * per, (t + 1) * per) of a set's part."""
    I64 = torch.int64
    address = address or (lambda x: x.data_ptr())
    t = lambda v: v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=I64)
    # a list's [F][3][2]: per feature (K, V^T) leading rows / row length / address; a timestep's rows are the leading rows over `per`
    # (a feature cache's lists hold F alone -- a K-shaped tensor: [F][3][1], and every record below is a K record)
    fact = lambda per, ptr, a, *b: [a.shape[0] // per] + [x.shape[1] for x in b] + [a.shape[1]] + [x.shape[2] for x in b] + [ptr(x) for x in (a,) + b]
    facts = lambda kv, per, ptr: torch.tensor([fact(per, ptr, *e) for e in kv], dtype=I64).view(len(kv), 3, -1)

    def runs(src, dst, exp, rows, cols, ldd, sinc, dinc):    # [...][7]: a record (lds = cols), then what its src / dst advance per entry / timestep slot
        return torch.stack(torch.broadcast_tensors(*[t(v) for v in (src, dst, exp, rows | (cols << 32), cols | (ldd << 32), sinc, dinc)]), dim=-1)
    F, T, P, esz = len(dst_kvs[0]), len(dst_kvs[0][0]), len(dst_kvs), dst_kvs[0][0][0].element_size()
    drows, dcols, dbase = torch.stack([facts(d, k * S, lambda x: x.data_ptr()) for d in dst_kvs]).unbind(2)   # [P][F][2]: (N_f, C_f), (C_f, ld_f)
    drows, dcols, dbase = drows[0], dcols[0], dbase.unsqueeze(1)
    dunit = drows * dcols * esz                                                                              # bytes of one slot
    tmpl = []                                                # per source, the records of timestep (entry 0, slot 0) of every set
    for kv, n, G, garments, gslots, exps in sources:
        su = esz if exps is None else 1                      # source / column unit in bytes
        rows, cols, base = facts(kv, n * G, address).unbind(1)                                               # (N'_f, C_f), (C_f, ld'_f)
        g, u = t(garments).view(-1, 1, 1), t(gslots).view(-1, 1, 1)
        unit = rows * cols * su                                                                              # bytes per (timestep, garment)
        dst = dbase + u * dunit
        exp = 0 if exps is None else address(exps) + 4 * (g * (T * F) + torch.arange(T * F).view(F, T))
        rec = runs(base + g * unit, dst, exp, rows, cols * su, dcols * su, G * unit, S * dunit)              # [P][U][F][2][7]
        if bool((dcols > cols).any()):                       # (K, V^T, the V^T zero run) of every feature, the last where there is a tail
            tail = runs(0, dst + cols * esz, 0, rows, (dcols - cols) * su, dcols * su, 0, S * dunit)[:, :, :, 1:]
            keep = torch.cat([torch.ones(F, 2, dtype=torch.bool), dcols[:, 1:] > cols[:, 1:]], dim=1)
            rec = torch.cat([rec, tail], dim=3)[keep.expand(P, len(garments), F, 3)]
        if T == 1 and bool((drows > rows).any()):            # (F, the zero ROW run) of every feature, the last where the garment has fewer rows
            tail = runs(0, dst + rows * cols * esz, 0, drows - rows, dcols * su, dcols * su, 0, S * dunit)
            keep = torch.cat([torch.ones(F, 1, dtype=torch.bool), drows > rows], dim=1)
            rec = torch.cat([rec, tail], dim=3)[keep.expand(P, len(garments), F, 2)]
        tmpl.append(rec.reshape(P, -1, 7))
    from . import ops
    T = torch.stack([ops.kv_pad_even(x) for x in torch.cat(tmpl, dim=1)])   # [P][per][7], per even
    rec = T[:, None, :, :5].repeat(1, len(entries), 1, 1)
    rec[..., :2] += torch.tensor([entries, tslots], dtype=I64).t().unsqueeze(1) * T[:, None, :, 5:]
    return rec.reshape(-1, 5), T.shape[1]


def cache_sources(gc, garments):
    """The sources (kv_records) that put garments `garments` of cache gc into garment slots 0, 1, ...: the cache's one list, or, shelved,
    one compact part each."""
    slots = list(range(len(garments)))
    if isinstance(gc, ShelvedGarmentCache):
        return [(gc.parts[g].kv, len(gc.timesteps), 1, [0], [u], gc.parts[g].exps if gc.packed else None) for u, g in zip(slots, garments)]
    return [(gc.kv, len(gc.timesteps), gc.G, garments, slots, gc.exps if gc.packed else None)]


def fill_records(src_kv, n, G, dst_kv, k, S, exps, entries, tslots, garments, gslots, address=None):
    """kv_records of ONE source of the slots' own size -- garments `garments` of the list src_kv (n timesteps of G; packed with exps, 16-bit
    with None) into garment slots `gslots` --: one record per (timestep, garment, feature, K | V^T), in that order."""
    return kv_records([(src_kv, n, G, garments, gslots, exps)], [dst_kv], k, S, entries, tslots, address)[0]


def shelf_records(parts, packed, dst_kv, k, S, entries, tslots, gslots, address=None):
    """kv_records of the COMPACT garments `parts` (G = 1 caches, all packed or all 16-bit), one source each, into the front of garment slots
    `gslots`, zero V^T tails included -- feature parts into a feature list dst_kv: zero ROW runs included.  -> (records, per)."""
    return kv_records([(p.kv, len(p.timesteps), 1, [0], [u], p.exps if packed else None) for p, u in zip(parts, gslots)],
                      [dst_kv], k, S, entries, tslots, address)


def staged_plan(gc, gindex, k, S, dst_kvs, device, arena=None, exps=None):
    """The copy-engine transport of a host-resident cache (pipeline.py, _cached_fill), as data: no kernel and no GPU call in here, so it runs on
    CPU tensors.  A block of c <= k timesteps of the call's U distinct garments (first-use order; all G without gindex) is first COPIED into a
    staging arena -- per source (cache_sources) a k-timestep list of its used garments in its own storage (uint8 of a packed cache, else its
    16-bit dtype), back to back -- and then PLACED by one idmvton_kv_place launch into slots 0 .. U - 1 of the first c timestep slots of a
    16-bit list of k timesteps of S slots.
    The arena is one flat uint8 tensor on `device`: k * (the used garments' source bytes per timestep), every tensor carved at a multiple of
    16 bytes.  Pass the `arena` / `exps` of an earlier plan to use them again (an arena that is too small is replaced).  dst_kvs: the
    destination lists, one per set.  ->
      arena, nbytes   the flat tensor and the bytes of it this plan uses
      exps            int32 [U][F][2] on `device` (None for a 16-bit source), exps_copies [(dst, src)] that fill it from the cache's exponents
      copies(idx)     [(dst, src)] tensor views that bring cache entries idx (a block, by value) into arena timestep slots 0 .. len(idx) - 1:
                      _fill_set's gather -- one pair per tensor when the entries are consecutive and there is no index (shelved: per part
                      tensor), else one per timestep and run of consecutive garments
      rec, per        the place records of every set (kv_records with the arena's lists as sources) and the records per timestep: set p's
                      block of c timesteps is records [p * k * per, p * k * per + c * per) -- a prefix, as the arena's addresses never change."""
    n = len(gc.timesteps)
    garments = list(range(gc.G)) if gindex is None else list(dict.fromkeys(gindex))
    U = len(garments)
    srcs = cache_sources(gc, garments)
    whole = gindex is None or isinstance(gc, ShelvedGarmentCache)   # every source list moves whole: all its garments, in its own order
    shapes = [[tuple(((a[0] // (n * G)) * k * len(gs),) + a[1:] for a in e[:-1]) + e[-1:] for e in kv_shapes(kv)] for kv, _, G, gs, _, _ in srcs]
    size = lambda sh, d: torch.Size(sh).numel() * torch.empty((), dtype=d).element_size()
    nbytes = sum(size(a, e[-1]) for lst in shapes for e in lst for a in e[:-1])
    if arena is None or arena.numel() < nbytes:
        arena = torch.empty(nbytes, dtype=torch.uint8, device=device)
    lists, at = [], 0
    for lst in shapes:
        kv = []
        for *shs, d in lst:
            pair = []
            for sh in shs:
                pair.append(arena[at:at + size(sh, d)].view(d).view(sh))
                at += size(sh, d)
            kv.append(tuple(pair))
        lists.append(kv)
    pairs = lambda dst, src: [(d, s) for dp, sp in zip(dst, src) for d, s in zip(dp, sp)]
    if gc.packed:
        exps = torch.empty((U, len(lists[0]), len(lists[0][0])), dtype=torch.int32, device=device) if exps is None else exps
        exps_copies = [(exps[us[0] + d0:us[0] + d0 + cc], ex[g0:g0 + cc]) for _, _, _, gs, us, ex in srcs for d0, g0, cc in index_runs(gs)]
    else:
        exps, exps_copies = None, []
    staged = [(lst, k, len(gs), list(range(len(gs))), us, exps[us[0]:us[0] + len(us)] if gc.packed else None) for lst, (_, _, _, gs, us, _) in zip(lists, srcs)]
    rec, per = kv_records(staged, dst_kvs, k, S, list(range(k)), list(range(k)))

    def copies(idx):
        idx = list(idx)
        c = len(idx)
        steps = [(0, idx[0], c)] if idx == list(range(idx[0], idx[0] + c)) else [(j, i, 1) for j, i in enumerate(idx)]
        if whole:
            return [p for lst, (kv, _, G, _, _, _) in zip(lists, srcs) for j0, i0, cc in steps
                    for p in pairs(timestep_run(lst, k, G, j0, cc), timestep_run(kv, n, G, i0, cc))]
        return [p for j, i in enumerate(idx) for d0, g0, cc in index_runs(garments)
                for p in pairs(slot_run(lists[0], k, U, j, d0, cc), slot_run(gc.kv, n, gc.G, i, g0, cc))]
    return dict(arena=arena, nbytes=nbytes, exps=exps, exps_copies=exps_copies, copies=copies, rec=rec, per=per, lists=lists)


class ShelvedGarmentCache(GarmentCache):
    """The garments of a batch as GarmentShelf.get hands them out: `parts`, G = 1 caches in host memory, each at its OWN compact size, declared
    for slots of one size -- (gh, gw) and slot_shapes [((N_f, C_f), (C_f, ld_f))] --; sizes[g] is garment g's own (gh, gw).  There is no
    single tensor list (kv is empty): the engine streams every part into the front of a set slot (module docstring), and what it computes is
    what it computes on `slotted(device)`.  The cache keeps its parts alive: removing a key from the shelf while a call is queued is safe.
    The parts may all be FEATURE caches (a GarmentShelf of storage "features" / "features-e4m3"): `features` is then true, slot_shapes are
    still the slot's ((N_f, C_f), (C_f, ld_f)) -- F has K's shape --, the engine streams each part's F into the front of a slot of a staging
    list with the zero rows behind it and projects the block; there is no slotted feature cache, so `slotted` is refused by name and
    TryonEngine.project_garment gives the K / V^T shelved cache to compare against."""

    def __init__(self, parts, *, gh, gw, slot_shapes, h=None, w=None):
        parts = list(parts)
        if len({p.features for p in parts}) > 1:
            raise ValueError("ShelvedGarmentCache: features mismatch (the parts are all feature caches or all K / V^T caches, never mixed)")
        if not parts or any(p.G != 1 or p.sizes is not None for p in parts) or len({p.packed for p in parts}) != 1:
            raise ValueError("ShelvedGarmentCache: needs at least one part, every part a G = 1 cache without `sizes`, all packed or all 16-bit")
        p0 = parts[0]
        super().__init__(G=len(parts), timesteps=p0.timesteps, h=p0.h if h is None else h, w=p0.w if w is None else w, gh=gh, gw=gw, dtype=p0.dtype,
                         attn_fp8=p0.attn_fp8, f8_exp=p0.f8_exp, weights_id=p0.weights_id, kv=[], sizes=[(p.gh, p.gw) for p in parts],
                         features=p0.features)
        self.parts = parts
        self.packed = p0.packed
        self.slot_shapes = [(tuple(a), tuple(b)) for a, b in slot_shapes]

    @property
    def nbytes(self):
        return sum(p.nbytes for p in self.parts)

    @property
    def host_resident(self):
        return True

    def __repr__(self):
        return (f"ShelvedGarmentCache(G={self.G}, steps={len(self.timesteps)}, latent={self.h}x{self.w}, slots of {self.gh}x{self.gw} holding "
                f"{sorted(set(self.sizes))}, dtype={self.dtype}, {'features, ' if self.features else ''}{'e4m3-packed, ' if self.packed else ''}"
                f"{self.nbytes / 2 ** 20:.1f} MiB compact in host memory)")

    def _with(self, parts, **kw):
        return ShelvedGarmentCache(parts, gh=self.gh, gw=self.gw, slot_shapes=self.slot_shapes, h=kw.get("h", self.h), w=kw.get("w", self.w))

    def for_person_size(self, h, w):
        return self._with(self.parts, h=h, w=w)              # the same parts, no copy

    def select(self, ids):
        """Garments ids[0], ids[1], ... as a new ShelvedGarmentCache on the SAME parts (they are never written in place); values may repeat."""
        return self._with([self.parts[g] for g in self.garment_ids(ids, len(ids))])

    def take(self, slot, device=None, pin_memory=False):
        """A copy of part `slot`: a compact G = 1 cache (packed if the shelf is), on `device` (default: host memory)."""
        if not 0 <= int(slot) < self.G:
            raise ValueError(f"GarmentCache take: slot mismatch ({slot} outside [0, G = {self.G}))")
        return self.parts[int(slot)].take(0, device, pin_memory)

    def slotted(self, device=None):
        """The 16-bit slotted GarmentCache that empty slots + put(g, take(g)) give (packed parts unpacked first), on `device` (default: host
        memory): what an engine call on this cache is compared against.  K rows no garment fills are zero.  Refused on feature parts: a
        cache with `sizes` and a tensor list holds K / V^T."""
        if self.features:
            raise ValueError("ShelvedGarmentCache slotted: features mismatch (there is no slotted feature cache: a cache with `sizes` and a tensor "
                             "list holds K / V^T -- engine.project_garment(<this cache>).slotted() is the slotted cache of these garments)")
        device = torch.device("cpu" if device is None else device)
        n, G = len(self.timesteps), self.G
        kv = [(torch.zeros((n * G * a[0], a[1]), dtype=self.dtype, device=device), torch.zeros((n * G, b[0], b[1]), dtype=self.dtype, device=device))
              for a, b in self.slot_shapes]
        out = GarmentCache(G=G, timesteps=self.timesteps, h=self.h, w=self.w, gh=self.gh, gw=self.gw, dtype=self.dtype, attn_fp8=self.attn_fp8,
                           f8_exp=self.f8_exp, weights_id=self.weights_id, kv=kv, sizes=[(self.gh, self.gw)] * G)
        for g, part in enumerate(self.parts):
            one = part.to(device)
            out.put(g, (one.unpack() if one.packed else one).for_person_size(self.h, self.w))
        return out

    def _no(self, name):
        raise ValueError(f"ShelvedGarmentCache {name}: a shelved cache has no single tensor list (its garments live in `parts`, each at its own "
                         "size); use slotted(), take() or select()")

    def put(self, slot, other): self._no("put")
    def save(self, path): self._no("save")
    def pack(self, exps=None): self._no("pack")
    def unpack(self): self._no("unpack")
    def repeat_garments(self, times): self._no("repeat_garments")
    def run(self, i0, c=1): self._no("run")
    def step(self, i): self._no("step")
    def to(self, device, pin_memory=False): self._no("to")

    @staticmethod
    def cat(caches):
        raise ValueError("ShelvedGarmentCache cat: a shelved cache has no single tensor list (its garments live in `parts`, each at its own "
                         "size); use GarmentShelf.get for the garments of a batch")


class GarmentShelf:
    """A host catalogue of garments of many sizes: key -> a COMPACT G = 1 cache in page-locked host memory (pageable where there is no GPU, so
    that the logic runs on a CPU), 16-bit (storage="native") or e4m3-packed ("e4m3": a 16-bit garment is packed on its way in, on the device
    it lives on).  `like` -- a cache with `sizes`, as TryonEngine.empty_garment_cache makes it, or any G = 1 cache -- fixes what every garment
    must agree with (timesteps, person size, dtype, attn_fp8, f8_exp, weights) and the SLOT size: every feature's K rows and V^T positions
    must fit it.  Only like's fields and shapes are kept, not its tensors.  max_bytes bounds the shelf: `get` evicts the least recently used
    garments that the batch does not name until it fits.
    storage="features" / "features-e4m3": a shelf of compact FEATURE caches (encode_garment(storage="features")), 16-bit / e4m3-packed --
    half / a quarter of the bytes of the K / V^T garment, in host RAM and over the host link.  `like` may then also be a G = 1 feature cache;
    either way the slot's F shape per feature is the slot's K shape (N_f, C_f), and a garment fits when its C_f is equal and its rows per
    timestep are at most N_f.  Kinds do not mix: a K / V^T garment into a feature shelf, and a feature garment into a K / V^T shelf, are
    ValueErrors naming `features`.
        shelf = GarmentShelf(pipe.empty_garment_cache(1, 1024, 768, 30), storage="e4m3")
        cache, index = shelf.get(["sku7", "sku3", "sku7"], encode=my_encode)
        out = pipe(cloth=cache, garment_index=index, ...)"""
    _IDENTITY = ("timesteps", "h", "w", "dtype", "attn_fp8", "f8_exp", "weights_id")

    def __init__(self, like, storage="native", max_bytes=None):
        if storage not in ("native", "e4m3", "features", "features-e4m3"):
            raise ValueError(f"GarmentShelf: storage={storage!r} (\"native\", \"e4m3\", \"features\" or \"features-e4m3\")")
        self.features = storage.startswith("features")       # the shelf's kind: compact feature caches, or compact K / V^T caches
        if isinstance(like, ShelvedGarmentCache):
            self.slot_shapes = list(like.slot_shapes)
        elif like.features:                                  # F [n * G * N_f][C_f]: K's shape, and V^T is (C_f, N_f) (project_garment)
            n = len(like.timesteps)
            self.slot_shapes = [((f.shape[0] // (n * like.G), f.shape[1]), (f.shape[1], f.shape[0] // (n * like.G))) for f, in like.kv]
        else:
            n = len(like.timesteps)
            self.slot_shapes = [((k.shape[0] // (n * like.G), k.shape[1]), (vt.shape[1], vt.shape[2])) for k, vt in like.kv]
        self.like = {f: getattr(like, f) for f in self._IDENTITY}
        self.gh, self.gw = like.gh, like.gw
        self.storage, self.max_bytes = storage, None if max_bytes is None else int(max_bytes)
        self._parts = {}                                     # key -> compact G = 1 cache, in use order: the first key is the least recently used
        self.stats = dict(hits=0, encoded=0, restored=0, evicted=0)

    def __contains__(self, key):
        return key in self._parts

    def __len__(self):
        return len(self._parts)

    @property
    def nbytes(self):
        return sum(p.nbytes for p in self._parts.values())

    def keys(self):
        """The keys, least recently used first."""
        return list(self._parts)

    def _compact(self, one):
        """`one` checked against the shelf and copied compact into host memory; ValueError naming the field otherwise."""
        if one.features and not self.features:
            raise ValueError(f"GarmentShelf add: features mismatch (a storage=\"{self.storage}\" shelf holds compact K / V^T garments; a feature "
                             "cache goes on a shelf of storage \"features\" / \"features-e4m3\" -- or engine.project_garment(features) gives "
                             "the K / V^T garment)")
        if self.features and not one.features:
            raise ValueError(f"GarmentShelf add: features mismatch (a storage=\"{self.storage}\" shelf holds compact feature caches; encode the "
                             "garment with storage=\"features\", or put its K / V^T on a \"native\" / \"e4m3\" shelf)")
        if one.G != 1:
            raise ValueError(f"GarmentShelf add: G mismatch (takes a cache of one garment, got G = {one.G})")
        if one.attn_fp8:
            raise ValueError("GarmentShelf add: attn_fp8 mismatch (an attn_fp8 garment holds e4m3 operands of the fp8 attention; a shelf is not "
                             "streamed by an attn_fp8 engine)")
        for f in self._IDENTITY:
            if getattr(one, f) != self.like[f]:
                raise ValueError(f"GarmentShelf add: {f} mismatch ({getattr(one, f)} against {self.like[f]})")
        if one.packed and not self.storage.endswith("e4m3"):
            raise ValueError(f"GarmentShelf add: packed mismatch (an e4m3-packed garment cannot go into a storage=\"{self.storage}\" shelf: unpack() "
                             "is not its 16-bit original)")
        if one.sizes is not None:                            # a one-slot slotted cache: the garment at its own compact size
            one = one.take(0)
        n = len(one.timesteps)
        if len(one.kv) != len(self.slot_shapes):
            raise ValueError(f"GarmentShelf add: does not fit ({len(one.kv)} features against {len(self.slot_shapes)})")
        for f, (e, ((N, C), (Cv, ld))) in enumerate(zip(one.kv, self.slot_shapes)):
            if self.features:
                if e[0].shape[1] != C or e[0].shape[0] // n > N:
                    raise ValueError(f"GarmentShelf add: does not fit (feature {f}: a garment of latent {one.gh}x{one.gw} has F rows "
                                     f"{e[0].shape[0] // n} x {e[0].shape[1]}, a slot of {self.gh}x{self.gw} holds {N} x {C})")
                continue
            k, vt = e
            if k.shape[1] != C or vt.shape[1] != Cv or k.shape[0] // n > N or vt.shape[2] > ld:
                raise ValueError(f"GarmentShelf add: does not fit (feature {f}: a garment of latent {one.gh}x{one.gw} has K rows {k.shape[0] // n} x "
                                 f"{k.shape[1]} and V^T {vt.shape[1]} x {vt.shape[2]}, a slot of {self.gh}x{self.gw} holds {N} x {C} and {Cv} x {ld})")
        if self.storage.endswith("e4m3") and not one.packed:
            one = one.pack()                                 # on the device it lives on
        return one.take(0, "cpu", pin_memory=torch.cuda.is_available())

    def add(self, key, one):
        """Put the one garment of `one` (G = 1, 16-bit or packed, of ANY size that fits the slot) on the shelf under `key`, compact, replacing
        what the key held.  Complete on return."""
        part = self._compact(one)
        self._parts.pop(key, None)
        self._parts[key] = part

    def remove(self, key):
        """Take a garment off the shelf (a ShelvedGarmentCache that names it keeps it alive)."""
        self._parts.pop(key, None)

    def get(self, keys, encode=None):
        """-> (ShelvedGarmentCache of the distinct garments of `keys` in first-use order, garment_index of the batch).  encode(key) -> a G = 1
        cache; it is called once per distinct key the shelf lacks (KeyError when there is none), and every garment is made before the shelf
        changes: nothing is added or evicted if encode raises.  With max_bytes, the least recently used garments the batch does not name are
        evicted until the shelf fits; ValueError when the batch alone exceeds the bound."""
        keys = list(keys)
        distinct = list(dict.fromkeys(keys))
        missing = [key for key in distinct if key not in self._parts]
        if missing and encode is None:
            raise KeyError(f"GarmentShelf: {missing[0]!r} is not on the shelf and no `encode` was given")
        new = {key: self._compact(encode(key)) for key in missing}
        batch = {key: new[key] if key in new else self._parts[key] for key in distinct}
        need = sum(p.nbytes for p in batch.values())
        if self.max_bytes is not None and need > self.max_bytes:
            raise ValueError(f"GarmentShelf: the batch alone holds {need} bytes, max_bytes is {self.max_bytes}")
        for key in distinct:                                 # most recently used: to the end
            self.stats["encoded" if key in new else "hits"] += 1
            self._parts.pop(key, None)
            self._parts[key] = batch[key]
        while self.max_bytes is not None and self.nbytes > self.max_bytes:
            del self._parts[next(k for k in self._parts if k not in batch)]
            self.stats["evicted"] += 1
        cache = ShelvedGarmentCache(list(batch.values()), gh=self.gh, gw=self.gw, slot_shapes=self.slot_shapes)
        return cache, [distinct.index(key) for key in keys]


class GarmentPool:
    """A resident pool: one `capacity`-slot GarmentCache and an LRU map key -> slot.  `get(keys, encode)` returns the garment_index list of a
    batch, after putting the garments the pool lacks into the least-recently-used slots that the batch does not itself need; evicted garments
    optionally go to pinned host memory and come back from there instead of being encoded again: spill=True keeps EVERY garment ever evicted
    (0.3-9.4 GB each at full size: unbounded), spill=<int> at most that many, dropping the one spilled longest ago; `drop(key)` frees one.
    mixed_sizes=True: the pool's cache is slotted -- `like` fixes the slot size, any garment that fits goes in, and a spilled garment has its own
    compact size on the host.  A slot's views are copied straight to and from the pinned tensors, with no temporary garment on the device.  Everything moves BEFORE the
    call -- a device-resident pool streams nothing during one -- and the pool's tensors never move, so an engine's graph states stay valid across swaps.
    resident="host": the pool's cache itself lives in page-locked host memory (pageable where there is no GPU, so that the logic runs on a CPU)
    and the engine streams every block of a call out of it (idmvton_kv_stream): capacity is bounded by host RAM, `get` and the LRU order are
    unchanged, `put` blocks (GarmentCache.put).  Not with spill (there is no second tier to spill to) or mixed_sizes (slotted host caches are
    not streamed).  The default "device" is the pool as it always was.
    A packed `like` (PackedGarmentCache) makes a packed pool: resident and spilled garments are e4m3 bytes + exponents, half the device and
    pinned host memory, and `encode` may return packed or 16-bit garments (the latter are packed on their way in); not with mixed_sizes.
        pool = GarmentPool(8, like=pipe.encode_garment(cloth=c0, ...))
        out = pipe(cloth=pool.cache, garment_index=pool.get(["sku7", "sku7", "sku3"], encode=my_encode), ...)"""

    def __init__(self, capacity, like, spill=False, mixed_sizes=False, resident="device"):
        if like.G != 1:
            raise ValueError(f"GarmentPool: `like` must hold one garment (G = {like.G})")
        if capacity < 1:
            raise ValueError(f"GarmentPool: capacity {capacity} < 1")
        if resident not in ("device", "host"):
            raise ValueError(f"GarmentPool: resident={resident!r} (\"device\" or \"host\")")
        if resident == "host" and (spill or mixed_sizes):
            raise ValueError(f"GarmentPool: resident=\"host\" cannot be combined with {'spill' if spill else 'mixed_sizes'} (the pool already lives in "
                             "host memory; slotted host caches are not streamed)")
        if like.features and mixed_sizes:
            raise ValueError("GarmentPool: features mismatch (mixed_sizes makes a slotted cache, which holds K / V^T; a feature cache cannot be its `like`)")
        self.resident = resident
        self.capacity, self.spill = int(capacity), bool(spill)
        self.host_capacity = None if spill is True or not spill else int(spill)      # garments kept on the host; None: no bound
        n = len(like.timesteps)
        if resident == "host":
            pin = torch.cuda.is_available()
            kv = [tuple(torch.empty((a[0] * self.capacity,) + tuple(a[1:]), dtype=e[-1], pin_memory=pin) for a in e[:-1]) for e in kv_shapes(like.kv)]
            carry = dict(exps=torch.zeros((self.capacity,) + tuple(like.exps.shape[1:]), dtype=torch.int32, pin_memory=pin)) if like.packed else {}
            self.cache = like._like(G=self.capacity, kv=kv, sizes=None, rows=None, **carry)
        elif mixed_sizes:
            # a slotted cache (module docstring): `like` fixes the slot size, `get` accepts every garment that fits, host copies are compact.
            # Slots are 16-bit, whatever `like` holds
            shapes = [(a, b, like.dtype if d == torch.uint8 else d) for a, b, d in kv_shapes(like.kv)]
            self.cache = like._like(G=self.capacity, kv=alloc_kv(shapes, 1, self.capacity, like.kv[0][0].device),
                                    sizes=[(like.gh, like.gw)] * self.capacity, rows=None)
        else:
            self.cache = like._like(G=self.capacity, kv=alloc_kv(kv_shapes(like.kv), 1, self.capacity, like.kv[0][0].device), sizes=None, rows=None)
        # alloc_kv scales the leading dimension of a list that holds n timesteps: [n * 1 ...] -> [n * capacity ...] is "capacity times as many"
        assert all(t.shape[0] == l.shape[0] * self.capacity for e, le in zip(self.cache.kv, like.kv) for t, l in zip(e, le))
        self._slot = {}                                      # key -> slot, in use order: the first key is the least recently used
        self._free = list(range(self.capacity))
        self.host = {}                                       # key -> spilled G = 1 cache in pinned host memory
        self.stats = dict(hits=0, encoded=0, restored=0, evicted=0)

    def __contains__(self, key):
        return key in self._slot

    def slots(self):
        """{key: slot} of the resident garments, least recently used first."""
        return dict(self._slot)

    def get(self, keys, encode=None):
        """-> the garment_index of a batch whose person i wears garment keys[i].  encode(key) -> a G = 1 GarmentCache like the pool's; it is
        called once per distinct key that is neither resident nor spilled.  ValueError when the batch has more distinct garments than slots."""
        keys = list(keys)
        distinct = list(dict.fromkeys(keys))
        if len(distinct) > self.capacity:
            raise ValueError(f"GarmentPool: the batch names {len(distinct)} distinct garments, the pool has capacity {self.capacity}")
        for key in distinct:
            if key in self._slot:
                self.stats["hits"] += 1
                self._slot[key] = self._slot.pop(key)        # most recently used: to the end
                continue
            if key not in self.host and encode is None:      # before anything is evicted for it
                raise KeyError(f"GarmentPool: {key!r} is not resident and no `encode` was given")
            # the garment first: if encode raises (out of memory, say) no slot has left `_free` and nothing was evicted for it
            restored = key in self.host
            one = self.host[key] if restored else encode(key)
            if self._free:
                slot = self._free.pop(0)
            else:                                            # the least recently used resident garment this batch does not name
                victim = next(k for k in self._slot if k not in distinct)
                slot = self._slot[victim]
                if self.spill and victim not in self.host:
                    self.host[victim] = self.cache.take(slot, "cpu", pin_memory=self.cache.kv[0][0].is_cuda)
                    while self.host_capacity is not None and len(self.host) > self.host_capacity:
                        del self.host[next(k for k in self.host if k != key)]      # spilled longest ago (never the one being restored)
                del self._slot[victim]
                self.stats["evicted"] += 1
            try:
                self.cache.put(slot, one)
            except BaseException:
                self._free.insert(0, slot)                   # the slot holds nothing valid, but it is not lost
                raise
            self._slot[key] = slot
            self.stats["restored" if restored else "encoded"] += 1
        return [self._slot[k] for k in keys]

    def drop(self, key):
        """Free the host copy of a spilled garment (a resident garment stays resident)."""
        self.host.pop(key, None)


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
