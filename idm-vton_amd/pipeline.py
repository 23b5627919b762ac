"""The try-on denoising engine: host mirror of StableDiffusionXLInpaintPipeline.__call__
(/root/reference/src/tryon_pipeline.py:1254-1894) for the path inference.py:397-414 takes, on the HIP kernels.

Per step (tryon_pipeline.py:1765-1866): pack 13-channel input -> GarmentNet -> TryonNet (garment K/V injected, CFG halves
in one batch, unconditional garment half in closed form) -> fused CFG + scheduler update.  Everything step-invariant is
computed once before the loop (time-embedding tables for every timestep, text / image-token K and V^T of all 140 attn2,
mask / masked-image / pose latents).  Optionally the step is captured into one hipGraph and replayed.

GarmentNet's inputs (cloth latent, cloth text, timestep) never depend on the latents, so the loop runs it for `garment_steps`
CONSECUTIVE TIMESTEPS IN ONE BATCH (batch = images x timesteps, each batch element with its own time embedding): the same
per-(image, timestep) arithmetic as the reference's one call per step (:1781-1787), but its GEMMs see 2-3x the rows (M = 1536
-> 4608 at the 1280-channel level), which is where the small-M projections of the loop lose their efficiency.  A "block" is
that GarmentNet batch plus the TryonNet steps that consume its features.  Blocks RAMP UP -- 1, 2, 4, then `garment_steps`
timesteps -- because only the first block's GarmentNet batch cannot hide behind TryonNet work (nothing runs before it): with a
one-timestep first block 7.5 ms of a call are exposed instead of the 45 ms of a six-timestep batch, and each later batch is
shorter than the TryonNet steps of the block before it.  Every batch runs at its exact size (no padded timesteps).

The same fact across calls: `encode_garment` runs the garment side alone (cloth VAE encode, GarmentNet batches in the same block schedule,
the K / V^T projections) and returns a GarmentCache; `prepare(cloth=<GarmentCache>)` then builds a call with no garment work at all, for
P persons on G cached garments (P % G == 0; the attention kernels read garment i % G for person i through a shared key segment) -- or, with
`garment_index=[...]`, for any P >= 1 persons of whom person i wears garment garment_index[i] of the cache (the kernels read the garment's
slot from a device table: an indexed key segment).  A cache with `sizes` (empty_garment_cache, GarmentPool(mixed_sizes=True)) holds garments
of several sizes in slots of one size; `prepare` then adds the per-person key counts of every garment feature as a second device table (a
ragged key segment), so one call -- and one graph state -- serves persons wearing garments of different sizes.

Structure of the loop.  The block order -- serial, or two streams with two alternating sets and two events per set -- is written once,
in `drive_blocks`, which knows nothing of graphs or caches (tests/test_loop_schedule_cpu.py checks its waits on stand-in streams).  An
execution form is the pair of callables it hands over:

                   garment(bi, p)                                    one TryonNet step (i = timestep, j = slot in set p)
    eager, live    _garment_side into set p                          _tryon_main on set p's views of slot j
    eager, cache   nothing to launch                                 _tryon_main on the cache's own views of entry gidx[i]
    graph, live    copy temb_gk[bi], replay ('garm', p, c)           copy tt / cf / nz, replay ('tryon', p, j)
    graph, cache   _cached_fill: the block's cache entries -> set p  as graph, live
Only a 16-bit cache on the device can be read in place.  A PACKED cache (GarmentCache.pack, encode_garment(storage="e4m3")) holds e4m3 bytes,
a HOST-RESIDENT one (page-locked CPU tensors: GarmentCache.to("cpu", pin_memory=True), GarmentPool(resident="host")) is not in HBM, and a
SHELVED one (ShelvedGarmentCache, GarmentShelf.get) holds compact garments of many sizes in page-locked memory: those go through 16-bit sets
in all four forms -- the eager forms then use sets too (one, or two with overlap), and with garment_index the P-slot sets and slot table of
the graph forms.  `_cached_fill` returns garment(bi, p) for every kind of cache, in _fill_set's place in drive_blocks' order (so every block
but the first crosses the host link behind the TryonNet steps of the block before it): ONE launch per block from a descriptor table built
and uploaded once per call -- idmvton_kv_unpack (packed, on the device), idmvton_kv_stream (host-resident), idmvton_kv_fill (shelved: the
zero V^T tail behind each garment too); key-count table, slot table, set shapes and graph key of a shelved cache are those of a
device-resident slotted cache of the same slot size.  The host-resident kinds have a second TRANSPORT, host_transport="copy" (opt-in per
call; "kernel" is the above): the copy engines bring a block's source bytes into a block-sized staging arena in HBM and ONE idmvton_kv_place
launch puts them into set p, so no kernel reads host memory beside TryonNet.  Same sets, same bits, same graph states.
A FEATURE cache (GarmentCache.features: GarmentNet's features in place of their K / V^T, half the bytes) goes through sets in every form too:
_cached_fill moves the block's features into a staging list of the set by the same means and projects them with one project_garment_kv.
A shelved cache may hold feature parts (GarmentShelf(storage="features")): the fill then also writes the zero rows behind each compact F.
With garment_index the two cache rows read through the table: eager on the cache's own views (nb = G, table = garment_index), graph on
P-slot sets into which _fill_set gathers the U distinct garments of the call (table = person -> set slot, a persistent buffer of the state).

Guidance is per person (prepare: guidance_scale / guidance_rescale as a float or one value per person).  A scalar scale without rescale is the
PLAIN state ([steps][4] coef table, idmvton_cfg_step); anything else the GUIDED state ([steps][3 + 2B] table, a `work` buffer,
idmvton_guided_step: the reference's rescale_noise_cfg fused into the step), with a graph state of its own.  uncond="skip" -- no person with
guidance -- runs the conditional branch alone: B TryonNet rows, the garment segment from batch 0 on, e = t; every form and every kind of cache
below serves it, since what they fill is the garment side.
Strength is per person too (prepare: strength as a float or one value per person).  A float is the call it always was; a sequence gives the
PERSON state ([steps][3 + 3B] table with an `active` column, idmvton_person_step): the loop runs the longest timestep list, and the step skips
the persons whose own list has not begun -- the only thing of a loop step that depends on the person.
Rows per step (prepare: rows="needed", opt-in, on a GarmentCache): a loop step runs only the TryonNet rows its persons need -- none for a
dormant person, no unconditional row for a person without guidance (_row_plans).  A call with something to skip is a ROW state
(st["rows"]: idmvton_pack_rows, TryonNet at R rows, idmvton_row_step; one graph state per call shape with captures per (R, a)); a call with
nothing to skip is the state it always was.  The garment side -- drive_blocks, the sets, _cached_fill -- does not know about it.

`denoise` asks once whether the call is live or on a cache, wraps the step in the per-step hooks (`trace`, `on_step`) and drives the
blocks.  The K / V^T layout of sets and cache (timestep-major) has one owner, garment_cache.timestep_run.
"""
import torch

from . import ops
from .garment_cache import (GarmentCache, PackedGarmentCache, ShelvedGarmentCache, alloc_kv, cache_sources, index_runs, kv_records, kv_shapes,
                            slot_run, staged_plan, timestep_run)
from .scheduler import StepScheduler, per_person


def drive_blocks(blocks, garment, tryon, main=None, side=None, ready=None, free=None):
    """The block loop, written once for every execution form.  garment(bi, p): put block bi's garment K / V^T into set p, on the current
    stream; tryon(bi, p): run the TryonNet steps of block bi against set p.  It knows nothing of graphs or caches.
    Serial order (no side stream): garment(bi, 0); tryon(bi, 0) per block, and a true return of tryon ends the loop (the per-step hook).
    Two-stream order (main = the current stream, side, two `ready` and two `free` events): block 0's garment work runs on main -- nothing
    to hide behind --, block bi+1's on side while TryonNet runs block bi on main; sets alternate by block parity.  ready[p]: set p is
    written (side -> main); free[p]: TryonNet is done reading set p (main -> side, before the block after next overwrites it)."""
    if side is None:
        for bi in range(len(blocks)):
            garment(bi, 0)
            if tryon(bi, 0):
                return
        return
    garment(0, 0)
    side.wait_stream(main)                                   # prepare()'s tensors and set 0 are complete
    for bi in range(len(blocks)):
        cur, nxt = bi & 1, (bi + 1) & 1
        if bi + 1 < len(blocks):
            with torch.cuda.stream(side):
                if bi >= 1:
                    side.wait_event(free[nxt])               # TryonNet block bi-1 is done reading set nxt
                garment(bi + 1, nxt)
                ready[nxt].record(side)
        if bi >= 1:
            main.wait_event(ready[cur])
        tryon(bi, cur)
        free[cur].record(main)
    main.wait_stream(side)


def _copy_state(G, st):
    """A new call's tensors -> the persistent buffers of a graph state, for every tensor the state owns and a captured graph reads (a
    GarmentCache state has no garment-side tensors)."""
    for name in ("latents", "cond", "cloth_k", "gix", "gnk"):
        if G.get(name) is not None:
            G[name].copy_(st[name])
    for name in ("ctx_t", "ctx_gk"):
        if name in G:
            for p, ent in st[name]["kv"].items():
                for kind, t in ent.items():
                    G[name]["kv"][p][kind].copy_(t)


def _is_attn1_kv(key):
    return ".attn1.to_k." in key or ".attn1.to_v." in key


class _Counters(dict):
    """TryonEngine.stats: a counter that has not counted yet reads 0 without being listed."""

    def __missing__(self, key):
        return 0


class TryonEngine:
    def __init__(self, unet, unet_encoder, vae, resampler=None, dtype=torch.bfloat16, device="cuda"):
        self.unet, self.unet_encoder, self.vae, self.resampler = unet, unet_encoder, vae, resampler
        self.dtype, self.device = dtype, torch.device(device)
        self._graphs = {}
        self._set_shapes = {}
        self._side = None
        self.garment_steps = 6                               # timesteps per GarmentNet batch (see the module docstring)
        self.ramp = True                                     # first blocks of 1, 2, 4 timesteps
        # garment_batches: GarmentNet batches launched or replayed by this engine (a call on a GarmentCache adds none); garment_set_copies: blocks
        # of cached K / V^T copied into a persistent set by the graph forms (on a packed cache: widened into one, by every form)
        # garment_stream_launches: blocks moved from a host-resident cache into a set (one idmvton_kv_stream / idmvton_kv_fill launch each)
        # garment_stage_copies / garment_stage_launches: host_transport="copy" -- tensor copies from a host-resident cache into the staging
        # arena (the copy engines), and blocks placed from the arena into a set (one idmvton_kv_place launch each)
        # garment_projections: blocks of a call on a FEATURE cache projected into a set (one project_garment_kv each, behind the block's
        # fill); it reads 0 and is listed from the first such block on (_Counters), so an engine that never saw a feature cache lists what
        # it always did
        self.stats = _Counters(garment_batches=0, garment_set_copies=0, garment_stream_launches=0, garment_stage_copies=0, garment_stage_launches=0)
        self._streaming = []                                 # [cache, event of its last queued fill]: host memory a queued launch still reads
        self._arenas = {}                                    # _cached_fill's staging arenas: one per call shape, reused across calls
        self._weights_id = None

    # -------------------------------------------------------------------------------------------- shared by prepare / encode_garment
    @staticmethod
    def _timesteps(scheduler, num_inference_steps, strength):
        sched = StepScheduler(scheduler)
        timesteps = sched.set_timesteps(num_inference_steps)                               # :1561
        init_t = min(int(num_inference_steps * strength), num_inference_steps)             # get_timesteps :987-995
        timesteps = timesteps[max(num_inference_steps - init_t, 0):]
        if len(timesteps) < 1:                                                             # :1568-1572
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline"
                             f"steps is {len(timesteps)} which is < 1 and not appropriate for this pipeline.")
        return sched, timesteps

    def _block_schedule(self, n):
        """-> (k, [(first step, steps)]): block sizes ramp 1, 2, 4, k, k, ... (module docstring)."""
        k = max(1, min(self.garment_steps, n))
        sizes, s0 = [], 0
        for c in (1, 2, 4):
            if c < k and s0 + c <= n and self.ramp:
                sizes.append(c); s0 += c
        while s0 < n:
            sizes.append(min(k, n - s0)); s0 += sizes[-1]
        blocks, s0 = [], 0
        for c in sizes:
            blocks.append((s0, c)); s0 += c
        return k, blocks

    def _garment_inputs(self, cloth_lat, text_embeds_cloth, timesteps, B):
        """GarmentNet's inputs for B garments over the call's timesteps, batched per block: batch index = j*B + b (timestep-major);
        temb_gk rows beyond a block's own c*B are never read."""
        dev, dt = self.device, self.dtype
        cloth_nhwc = ops.to_nhwc(cloth_lat, dt, cpad=self.unet_encoder.cin_pad)
        ctx_g = self.unet_encoder.encode_context(text_embeds_cloth.to(dev))
        temb_g = self.unet_encoder.time_embeddings(timesteps, B)
        n = len(timesteps)
        k, blocks = self._block_schedule(n)
        tidx = torch.tensor([[min(s0 + j, n - 1) for j in range(k)] for s0, _ in blocks], device=dev)
        temb_gk = temb_g[tidx].reshape(len(blocks), k * B, -1).contiguous()
        cloth_k = cloth_nhwc.repeat(k, 1, 1).contiguous()
        ctx_gk = ctx_g if k == 1 else self.unet_encoder.encode_context(text_embeds_cloth.to(dev).repeat(k, 1, 1))
        return dict(cloth=cloth_nhwc, ctx_g=ctx_g, temb_g=temb_g, k=k, blocks=blocks, temb_gk=temb_gk, cloth_k=cloth_k, ctx_gk=ctx_gk)

    @staticmethod
    def _garment_latent_size(cloth):
        """The garment runs at the cloth image's own size (the reference encodes it as it is, tryon_pipeline.py:1654, and its tokens meet the
        person's only along the token axis, attentionhacked_tryon.py:334): -> latent (gh, gw)."""
        Hg, Wg = cloth.shape[-2:]
        if Hg % 8 or Wg % 8:
            raise ValueError(f"`cloth` height and width have to be divisible by 8 but are {Hg} and {Wg}.")
        return Hg // 8, Wg // 8

    @staticmethod
    def _set_key(st):
        """What the shapes of a persistent garment set depend on: garments, the garment's latent size, timesteps per batch -- and an
        element of its own for a call that runs the conditional branch alone (uncond="skip")."""
        return (st["B"], st["gh"], st["gw"], st["k"]) + (("cond-only",) if st.get("branches", 2) == 1 else ())

    @staticmethod
    def _kind(st):
        """The kind of a call's state or of a graph state, named in this one place: "rows" (a row plan: pack_rows, TryonNet at R rows,
        row_step), "person" (a strength per person: person_step), "guided" (guidance per person, or the conditional branch alone:
        guided_step) or "plain" (cfg_step).  It is the suffix of the graph key, the step _tryon_main launches and what a step counts."""
        if st.get("rows") is not None:                       # (a graph state's is a dict that fills on first use: empty, and a row state)
            return "rows"
        if st.get("person"):
            return "person"
        return "guided" if st.get("guided") else "plain"

    @staticmethod
    def _graph_key(st, live):
        """One persistent graph state per shape of a call: persons, person latent size, garment latent size, block size, step noise, and on a
        GarmentCache its garment count -- or, with garment_index, nothing more: the sets of an indexed state have one slot per PERSON, so one
        state serves every pool size and every assignment.  A cache with `sizes` adds "ragged" (its forwards read a key-count table that a plain
        state's captures do not have); gh, gw are then the SLOT size, and the garments' own sizes are not in the key.  A GUIDED state (per-person
        guidance: another `cf` width, a `work` buffer, idmvton_guided_step in its captures) adds ("guided", branches) -- branches 1 being
        uncond="skip", whose captures run B TryonNet rows; a plain state's key is what it always was.  A PERSON state (a strength per
        person: a `cf` of 3 + 3B, idmvton_person_step in its captures -- which takes the guidance per person too) has ("person", branches) in
        that place, whatever its guidance."""
        kind = TryonEngine._kind(st)                         # (a ROW state: rows="needed" with something to skip; captures per (R, a) inside it)
        guided = ((kind, st.get("branches", 2)),) if kind != "plain" else ()
        if live:
            return (st["B"], st["h"], st["w"], st["gh"], st["gw"], st["k"], st["steps_noise"] is not None) + guided
        return (st["B"], st["h"], st["w"], st["gh"], st["gw"], st["k"], st["steps_noise"] is not None, "cached",
                "indexed" if st.get("gindex") is not None else st["gcache"].G) + (("ragged",) if st.get("gnk") is not None else ()) + guided

    UNCOND = ("run", "skip")

    @staticmethod
    def _guidance(B, guidance_scale, guidance_rescale, uncond):
        """prepare's guidance arguments -> (g per person, phi per person, guided state?, skip the unconditional rows?): checked here, before
        anything is launched.  A person with g <= 1 gets g = 1 and phi = 0 (no guidance, and the rescale is applied under CFG only)."""
        if uncond not in TryonEngine.UNCOND:
            raise ValueError(f"uncond={uncond!r}: \"run\" (the batched step, guidance 1 for a person without guidance) or \"skip\" (the "
                             "conditional branch alone, when no person has guidance)")
        g, g_seq = per_person(guidance_scale, B, "guidance_scale")
        phi, phi_seq = per_person(guidance_rescale, B, "guidance_rescale")
        if any(not 0.0 <= p <= 1.0 for p in phi):
            raise ValueError(f"`guidance_rescale` lies in [0, 1], got {guidance_rescale!r}")
        skip = uncond == "skip"
        if skip and any(x > 1 for x in g):
            raise ValueError(f"uncond=\"skip\" runs the conditional branch alone, which needs guidance_scale <= 1 for every person; got "
                             f"{guidance_scale!r} (uncond=\"run\" runs both branches)")
        phi = [p if x > 1 else 0.0 for x, p in zip(g, phi)]
        g = [x if x > 1 else 1.0 for x in g]
        guided = skip or g_seq or phi_seq or guidance_rescale != 0.0
        return g, phi, guided, skip

    @staticmethod
    def _person_steps(B, strength, n):
        """prepare's `strength` -> (None, None) for a float: the call it always was -- or, for a sequence of B floats in (0, 1], (the
        strengths, person i's own step count n_i = min(int(n * s_i), n)): checked here, before anything is launched."""
        if getattr(strength, "ndim", None) == 0 or not (hasattr(strength, "__len__") or hasattr(strength, "__iter__")):
            return None, None
        s_b, _ = per_person(strength, B, "strength")
        if any(not 0.0 < s <= 1.0 for s in s_b):
            raise ValueError(f"`strength` lies in (0, 1] for every person, got {strength!r}")
        n_b = [min(int(n * s), n) for s in s_b]
        for s, n_i in zip(s_b, n_b):
            if n_i < 1:                                                                    # :1568-1572, for the person it is true of
                raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {s}, the number of pipeline"
                                 f"steps is {n_i} which is < 1 and not appropriate for this pipeline.")
        return s_b, n_b

    ROWS = ("all", "needed")

    @staticmethod
    def _row_plans(B, n_b, g_b, n_max):
        """The row plan of every loop step of a call under rows="needed" -> (plan index per step, the distinct plans), or None when no
        step has fewer than 2B rows to run that today's states do not already skip.  n_b: the persons' own step counts (None: everyone
        takes all n_max steps); g_b: their guidance scales.  Person i is active in loop steps [n_max - n_i, n_max) (the person state's
        rule).  Step j runs the unconditional rows of the active persons with g > 1, then the conditional rows of the active persons, both
        in ascending person order.  A plan: persons (A, a of them), uncond (u of them), R = u + a, row_person[R], urow[B] / crow[B] (a
        person's row, or -1) and full_rows[R] (the same rows' indices in the [uncond B | cond B] layout).  Activity is nested over the loop
        and g is fixed, so there are at most B distinct plans and a shape (R, a) names one.
        None: every person active in every step and either everyone with g > 1 (the plain / guided / person state) or no one (the
        conditional branch alone: today's branches = 1 state)."""
        n_b = [n_max] * B if n_b is None else list(n_b)
        cfg = [g > 1 for g in g_b]
        if all(n == n_max for n in n_b) and (all(cfg) or not any(cfg)):
            return None
        index, plans, seen = [], [], {}
        for j in range(n_max):
            A = [i for i in range(B) if j >= n_max - n_b[i]]
            U = [i for i in A if cfg[i]]
            key = (len(U) + len(A), len(A))
            if key not in seen:
                urow, crow = [-1] * B, [-1] * B
                for r, i in enumerate(U):
                    urow[i] = r
                for r, i in enumerate(A):
                    crow[i] = len(U) + r
                seen[key] = len(plans)
                plans.append(dict(persons=A, uncond=U, a=len(A), u=len(U), R=len(U) + len(A), row_person=U + A, urow=urow, crow=crow,
                                  full_rows=U + [B + i for i in A]))
            index.append(seen[key])
        return index, plans

    def weights_identity(self):
        """What a GarmentCache depends on besides its inputs: every GarmentNet weight, and TryonNet's attn1.to_k / to_v (the projections of
        project_garment_kv), as stored (dtype included)."""
        if self._weights_id is None:
            self._weights_id = self.unet_encoder.weights_id() + ":" + self.unet.weights_id(_is_attn1_kv)
        return self._weights_id

    # -------------------------------------------------------------------------------------------- the garment side, once
    @torch.no_grad()
    def encode_garment(self, *, cloth, text_embeds_cloth, noise_cloth, num_inference_steps, scheduler="ddpm", strength=1.0,
                       height=None, width=None, storage="native"):
        """The garment side of a call for G = cloth.shape[0] garments, computed once: -> GarmentCache for `prepare(cloth=<it>)`.
        storage="e4m3": -> a PackedGarmentCache (garment_cache.py: e4m3 bytes + one exponent per garment, feature and tensor), bit-equal to
        encode_garment(storage="native").pack() without that cache ever being resident.  The exponent needs the largest |x| over ALL
        timesteps, so the block schedule runs TWICE into one block-sized 16-bit set: the first pass keeps the running maxima only, the second
        packs each block into the cache's bytes under the final exponents (the launches are deterministic: both passes produce the same
        bits).  Peak device memory beyond the weights: the packed cache (half the native one) + ONE block of 16-bit K / V^T and features
        (garment_steps of n timesteps: 6 / 30 of the native cache at the default schedule) + that block's bytes once more on their way
        into the cache (half the block) + one fp32 copy of the largest single tensor of the block while it is scaled.  Costs a second run of the GarmentNet batches; encoding is not on a call's path.
        cloth in [-1,1] [G,3,Hg,Wg], any size divisible by 8: the garment runs at its own latent (gh, gw) = (Hg / 8, Wg / 8); noise_cloth: the
        posterior draw of the cloth encode, [G,4,gh,gw] fp32 (noise['cloth'] of an uncached call).  height / width: the PERSON size the cache is
        declared for (default: the cloth's); GarmentCache.for_person_size re-declares it, the K / V^T do not depend on it.
        Runs what the loop runs for the garment side -- cloth VAE encode, encode_context, time_embeddings, and per block the GarmentNet batch
        + project_garment_kv -- IN THE SAME BLOCK SCHEDULE (1, 2, 4, k, k, ...) and at the same batch sizes as an uncached call with G
        persons and this num_inference_steps / strength, so every launch is the launch that call makes and the cached K / V^T are its bits.
        For the same reason a cloth of the person's size goes through the VAE encoder in the third slot of a 3G-image pass, where an uncached
        call encodes it (prepare: [masked image | pose | cloth]): per image the arithmetic does not depend on the batch, but which GEMM tile
        runs may.  A cloth of another size has a pass of its own there, and here.
        storage="features": -> a FEATURE cache (GarmentCache.features): the same preamble and block schedule, but each block's GarmentNet
        features F are kept -- GarmentNet writes them into the cache's own rows -- in place of their K / V^T: exactly half the bytes, no loss.
        A call on it projects every block behind its fill (_cached_fill), and project_garment gives the native cache.
        storage="features-e4m3": encode_garment(storage="features").pack(), bit for bit -- a quarter of the native bytes.  One 16-bit
        feature cache is resident during the encode: half of what "native" needs (the exponents need the largest |x| over all timesteps).
        An attn_fp8 engine refuses both (its sets mix e4m3 and 16-bit tensors): ValueError naming attn_fp8, before anything is launched."""
        if storage not in ("native", "e4m3", "features", "features-e4m3"):
            raise ValueError(f"encode_garment: storage={storage!r} (\"native\", \"e4m3\", \"features\" or \"features-e4m3\")")
        if storage.startswith("features"):
            self._refuse_features_fp8("encode_garment(storage=\"%s\")" % storage)
        dev = self.device
        f32 = lambda t: t.to(dev, torch.float32).contiguous()
        cloth, nz = f32(cloth), f32(noise_cloth)
        G = cloth.shape[0]
        Hg, Wg = cloth.shape[-2:]
        H = height or Hg
        W = width or Wg
        if H % 8 or W % 8:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {H} and {W}.")
        gh, gw = self._garment_latent_size(cloth)
        h, w = H // 8, W // 8
        _, timesteps = self._timesteps(scheduler, num_inference_steps, strength)
        if (Hg, Wg) == (H, W):
            cloth_lat = self.vae.encode_sample(torch.cat([cloth, cloth, cloth]), torch.cat([nz, nz, nz]))[2 * G:]
        else:
            cloth_lat = self.vae.encode_sample(cloth, nz)
        gs = dict(B=G, gh=gh, gw=gw, **self._garment_inputs(cloth_lat, text_embeds_cloth, timesteps, G))
        n, k = len(timesteps), gs["k"]
        fs, ks = self._discover_set_shapes(gs)
        feats = [torch.empty(sh, dtype=self.dtype, device=dev) for sh in fs] if not storage.startswith("features") else None
        if storage == "e4m3":
            return self._encode_packed(gs, feats, ks, timesteps, h, w)
        meta = dict(G=G, timesteps=timesteps, h=h, w=w, gh=gh, gw=gw, dtype=self.dtype, attn_fp8=self.unet.attn_fp8, f8_exp=self.unet.f8_exp,
                    weights_id=self.weights_identity())
        if storage != "native":                              # each block's features land in the cache's own rows; nothing is projected
            F = alloc_kv([((sh[0] * sh[1], sh[2]), self.dtype) for sh in fs], k, n, dev)
            for bi, (s0, c) in enumerate(gs["blocks"]):
                self._garment_feats(gs, gs["temb_gk"][bi], self._feature_views(timestep_run(F, n, G, s0, c), c * G), c)
            fc = GarmentCache(kv=F, features=True, **meta)
            return fc.pack() if storage == "features-e4m3" else fc
        kv = alloc_kv(ks, k, n, dev)
        for bi, (s0, c) in enumerate(gs["blocks"]):          # each block's projections land in the cache's own rows
            self._garment_side(gs, gs["temb_gk"][bi], dict(feats=feats, kv=timestep_run(kv, n, G, s0, c)), c)
        return GarmentCache(kv=kv, **meta)

    def _refuse_features_fp8(self, what):
        if self.unet.attn_fp8:
            raise ValueError(f"{what}: attn_fp8 mismatch (an attn_fp8 engine neither makes nor takes a feature cache: its sets mix e4m3 and 16-bit "
                             "tensors; encode K / V^T with storage=\"native\")")

    @staticmethod
    def _feature_views(entries, Bg):
        """Timestep-major feature entries [(F [Bg * N_f][C_f],)] -> GarmentNet's feature list [F as [Bg][N_f][C_f]]: what feats_buf and
        project_garment_kv take."""
        return [f.view(Bg, f.shape[0] // Bg, f.shape[1]) for f, in entries]

    @torch.no_grad()
    def project_garment(self, features):
        """A feature cache -> the native GarmentCache (a new one, on this engine's device): attn1.to_k / to_v applied to its features in the
        encode's block schedule at the cache's G, so every projection launch is the one encode_garment(storage="native") makes and the K / V^T
        are its bits.  A packed feature cache is unpacked first (exactly) and gives the K / V^T of its widened values.  The migration path
        from features to K / V^T, and what a call on a feature cache is compared against.
        A ShelvedGarmentCache of feature parts (GarmentShelf(storage="features" / "features-e4m3").get) gives the K / V^T ShelvedGarmentCache
        of the same garments for the same slots: every part is projected at its OWN size as above and compacted into page-locked memory
        (16-bit parts, whatever the source's storage)."""
        if not isinstance(features, GarmentCache) or not features.features:
            raise ValueError("project_garment: features mismatch (takes a feature cache: encode_garment(storage=\"features\"))")
        self._refuse_features_fp8("project_garment")
        if isinstance(features, ShelvedGarmentCache):
            parts = [self.project_garment(part).take(0, "cpu", pin_memory=torch.cuda.is_available()) for part in features.parts]
            return ShelvedGarmentCache(parts, gh=features.gh, gw=features.gw, slot_shapes=features.slot_shapes, h=features.h, w=features.w)
        if features.dtype != self.dtype or features.weights_id != self.weights_identity():
            raise ValueError(f"project_garment: {'dtype' if features.dtype != self.dtype else 'weights'} mismatch (the cache was built in "
                             f"{features.dtype} with weights {features.weights_id}; the engine runs {self.dtype} with {self.weights_identity()})")
        fc = features.to(self.device)
        fc = fc.unpack() if fc.packed else fc
        n, G = len(fc.timesteps), fc.G
        k, blocks = self._block_schedule(n)
        kv = alloc_kv(self._feature_kv_shapes(fc, G), n, n, self.device)
        for s0, c in blocks:
            self.unet.project_garment_kv(self._feature_views(fc.run(s0, c), c * G), out=timestep_run(kv, n, G, s0, c))
        return GarmentCache(**fc._args(kv=kv, features=False))

    @staticmethod
    def _feature_kv_shapes(fc, slots):
        """(K, V^T) shapes of a list that holds the n timesteps of `slots` garments of feature cache fc, derived from F's: K is F's shape,
        V^T (C_f, N_f) per garment and timestep."""
        n = len(fc.timesteps)
        return [((f.shape[0] // fc.G * slots, f.shape[1]), (n * slots, f.shape[1], f.shape[0] // (n * fc.G)), fc.dtype) for f, in fc.kv]

    def _encode_packed(self, gs, feats, ks, timesteps, h, w):
        """encode_garment(storage="e4m3") after the shared preamble: see its docstring."""
        if self.unet.attn_fp8:
            raise ValueError("encode_garment(storage=\"e4m3\"): an attn_fp8 engine's cache cannot be packed (its features already are e4m3 operands)")
        G, n, k, dev = gs["B"], len(timesteps), gs["k"], self.device
        blk = alloc_kv(ks, k, k, dev)                        # one block of 16-bit K / V^T, reused by every batch of both passes
        meta = dict(G=G, timesteps=timesteps, h=h, w=w, gh=gs["gh"], gw=gs["gw"], dtype=self.dtype, attn_fp8=False, f8_exp=self.unet.f8_exp,
                    weights_id=self.weights_identity())
        amax = None
        for bi, (s0, c) in enumerate(gs["blocks"]):          # pass 1: the largest |x| per (garment, feature, tensor), as exponents' input
            self._garment_side(gs, gs["temb_gk"][bi], dict(feats=feats, kv=timestep_run(blk, k, G, 0, c)), c)
            m = torch.stack([torch.stack([t.reshape(c, G, -1).abs().amax(dim=(0, 2)).float() for t in kvf], dim=-1)
                             for kvf in timestep_run(blk, k, G, 0, c)], dim=1)
            amax = m if amax is None else torch.maximum(amax, m)
        from .garment_cache import pack_exponent
        exps = pack_exponent(amax)                           # [G][F][2], on the device, no host sync
        kv = alloc_kv([(a, b, torch.uint8) for a, b, _ in ks], k, n, dev)
        for bi, (s0, c) in enumerate(gs["blocks"]):          # pass 2: the same batches, packed into the cache's own rows
            views = timestep_run(blk, k, G, 0, c)
            self._garment_side(gs, gs["temb_gk"][bi], dict(feats=feats, kv=views), c)
            part = GarmentCache(**{**meta, "timesteps": timesteps[s0:s0 + c], "kv": views}).pack(exps)
            for (dk, dv), (sk, sv) in zip(timestep_run(kv, n, G, s0, c), part.kv):
                dk.copy_(sk)
                dv.copy_(sv)
        self.stats["garment_batches"] -= len(gs["blocks"])   # counted once: the batches of the cache
        return PackedGarmentCache(exps=exps, kv=kv, **meta)

    def empty_garment_cache(self, G, garment_height, garment_width, num_inference_steps, scheduler="ddpm", strength=1.0, height=None, width=None):
        """A slotted GarmentCache (one with `sizes`) of G uninitialised slots laid out for garments of garment_height x garment_width: what
        `put` fills with garments of that size or any smaller one, and what a GarmentPool(mixed_sizes=True) takes as `like` -- a pool for a
        maximum garment size without encoding a garment of it.  Nothing is encoded and nothing is launched: feature f of a slot has
        round16(feature_tokens(gh, gw)[f]) rows of TryonNet's attn1 width, 16-bit (an fp8 engine quantises a slot per launch).  height /
        width: the PERSON size the cache is declared for (default: the garment's), as in encode_garment."""
        if garment_height % 8 or garment_width % 8:
            raise ValueError(f"`garment_height` and `garment_width` have to be divisible by 8 but are {garment_height} and {garment_width}.")
        H, W = height or garment_height, width or garment_width
        if H % 8 or W % 8:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {H} and {W}.")
        if G < 1:
            raise ValueError(f"empty_garment_cache: G = {G} < 1")
        gh, gw = garment_height // 8, garment_width // 8
        _, timesteps = self._timesteps(scheduler, num_inference_steps, strength)
        n = len(timesteps)
        kv = []
        for blk, tokens in zip(self.unet.block_order, self.unet.feature_tokens(gh, gw)):
            C, N = blk["qkv"].shape[1], ops.round16(tokens)
            kv.append((torch.empty(n * G * N, C, dtype=self.dtype, device=self.device), torch.empty(n * G, C, N, dtype=self.dtype, device=self.device)))
        return GarmentCache(G=G, timesteps=timesteps, h=H // 8, w=W // 8, gh=gh, gw=gw, dtype=self.dtype, attn_fp8=self.unet.attn_fp8,
                            f8_exp=self.unet.f8_exp, weights_id=self.weights_identity(), kv=kv, sizes=[(gh, gw)] * G)

    # -------------------------------------------------------------------------------------------- preparation
    @torch.no_grad()
    def prepare(self, *, image, mask_image, pose_img, cloth, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds,
                negative_pooled_prompt_embeds, text_embeds_cloth, noise, num_inference_steps, guidance_scale,
                ip_hidden_states=None, image_embeds=None, scheduler="ddpm", height=None, width=None, strength=1.0,
                image_dtype=None, garment_index=None, guidance_rescale=0.0, uncond="run", rows="all"):
        """Everything before the loop (tryon_pipeline.py:1495-1762).  image in [0,1]; pose_img / cloth in [-1,1];
        noise: dict(latents, masked, pose [B,4,h,w] fp32; cloth [B,4,gh,gw] fp32; steps [n,B,4,h,w] fp32 or None; image [B,4,h,w] when
        strength < 1) -- RNG order SURVEY A.4.
        cloth: [B,3,Hg,Wg] of any size divisible by 8 -- the garment runs at its own latent (gh, gw) = (Hg / 8, Wg / 8), as in the reference,
        which encodes the cloth as it is (:1654) and joins its tokens to the person's along the token axis only.  What another garment size
        does to image quality is not evaluated here (no trained weights): the engine runs what the reference runs.
        strength < 1 (:987-995, 883-893): the last int(n*strength) timesteps, starting from add_noise(encode(image), noise, t_0).
        guidance_scale <= 1 (:440-442: no classifier-free guidance): the reference runs the conditional branch alone; here the
        batched step runs with guidance 1 -- u + 1*(t - u) = t to one fp32 rounding -- so negative_* may be None and
        ip_hidden_states / image_embeds may hold the B conditional rows only.
        cloth = a GarmentCache (encode_garment) of G garments: no garment work in this call -- no cloth encode, no GarmentNet inputs;
        text_embeds_cloth and noise['cloth'] may be None.  B = image.shape[0] persons, B % G == 0, person i wears garment i % G.  A cache
        that does not cover the call (timestep, resolution, dtype mode, weights, B % G) raises ValueError before anything is launched.
        garment_index (with a GarmentCache only): B ints in [0, G), person i wears garment garment_index[i] -- any B >= 1, values may repeat,
        no B % G rule; the cache is a pool, and G may exceed B.  A cache with `sizes` (garments of several sizes in slots of one size) needs
        garment_index: which size a person's garment has follows from the slot it names.
        A HOST-RESIDENT cache (CPU tensors) is streamed into the sets block by block during the call (_cached_fill); every tensor -- and a
        packed cache's `exps` -- must be page-locked (pin_memory), the cache must not have `sizes`, and the engine must not be attn_fp8: each
        a ValueError naming the field, before anything is launched.  A ShelvedGarmentCache (GarmentShelf.get) is the host-resident cache WITH
        sizes: garment_index is required, every part and every part's `exps` must be page-locked, the engine must not be attn_fp8; its
        parts are compact K / V^T caches or compact feature caches (GarmentShelf(storage="features" / "features-e4m3")).
        guidance_scale / guidance_rescale: a float, or a sequence of B floats -- one per person, as the garment is (a service need not split
        a batch by them).  guidance_rescale (rescale_noise_cfg, :101-113, applied as :1818-1820: under CFG only) lies in [0, 1].  A person
        with g <= 1 runs with g = 1 and without rescale.  A scalar guidance_scale with guidance_rescale == 0 (a scalar) and uncond="run" gives
        the PLAIN state: the [steps][4] coef table and idmvton_cfg_step, as ever.  Anything else gives the GUIDED state: a [steps][3 + 2B]
        coef table, a `work` buffer and idmvton_guided_step (st["guided"]), with a graph state of its own.
        uncond="skip" (only when every person has g <= 1): the reference's form of a call without guidance (:1229-1230) -- the conditional
        branch ALONE: B TryonNet rows instead of 2B (x_in, cond, temb_t, ctx_t, the key-count table), the garment segment from batch 0 on,
        e = t in the step.  negative_* are not read; ip_hidden_states / image_embeds may hold B rows or 2B (the first B are dropped).
        uncond="run" (the default) keeps the batched step with guidance 1 for such a call.
        A sequence of the wrong length, a rescale outside [0, 1], an unknown `uncond` or uncond="skip" with a g > 1 is a ValueError naming
        the argument, before anything is launched.
        strength: a float -- the call it always was: same state, table, kernel and graph key --, or a sequence of B floats in (0, 1]: one
        batch mixes img2img depths.  Person i's step count is n_i = min(int(n * s_i), n); the loop runs the timestep list of the largest,
        n_max (every person's list is a suffix of it, so the cache, the time embeddings and the block schedule are the loop's, not a
        person's); person i is DORMANT in loop steps [0, n_max - n_i) -- its latents hold its own start, add_noise(encode(image_i),
        noise_i, its first timestep) or noise_i at s_i == 1, and the step neither reads nor writes them -- and active after that.  Person
        i's result is bit-identical to row i of the same batch run with the scalar strength s_i.  Dormant rows still run through TryonNet
        and their eps is dropped: a call costs n_max full-batch steps, whatever the other strengths (running an active prefix of the batch
        alone is not done).  noise['steps'] is aligned to LOOP steps, [n_max, B, 4, h, w]: the scalar call at s_i gets
        noise['steps'][n_max - n_i:]; a dormant person's rows are not read.  noise['image'] is needed when some s_i < 1 (unless
        latents_given).  A sequence gives the PERSON state (st["person"]): a [steps][3 + 3B] coef table {.., g, phi, active},
        idmvton_person_step -- which applies guidance_scale / guidance_rescale per person too, and runs under uncond="skip" -- and a graph
        state of its own; stats["person_steps"] counts its steps.  A wrong length, a value outside (0, 1], NaN or an n_i < 1 (the
        reference's message) is a ValueError naming `strength`, before anything is launched.  A step count per person stays out: a garment
        cache is keyed to one timestep list.
        rows: "all" (the default: nothing changes) or "needed" (opt-in, on a GarmentCache): loop step j runs only the TryonNet rows its
        persons need -- the unconditional rows of the persons active at j with g > 1, then the conditional rows of the persons active
        at j, each in ascending person order (_row_plans).  A person with g <= 1 gets e = t, what uncond="skip" computes: its bits may
        differ from rows="all" by one fp32 rounding of eps, and at sizes where the GEMM tile follows the row count a person's bits follow
        the rows its steps ran with, which is why this is opt-in.  A call with nothing to skip is the state it is today,
        key for key and kernel for kernel (all g <= 1 and nobody dormant: the branches = 1 state of uncond="skip"); a call in which some
        step has fewer than 2B rows is a ROW state: st["rows"] = the plans and the step -> plan map, `cond` [B][hw][9], a guided coef
        table, idmvton_pack_rows / idmvton_row_step, TryonNet at R rows, a graph state of its own.  The full-layout context and time
        embeddings are computed as ever (2B rows: the bits of rows="all") and gathered per plan.  A cache without garment_index is read
        through the index i % G.  The garment fills are untouched: all B persons' garments are moved for every step, a dormant
        person's slot is not read.  stats["tryon_rows"] / ["row_steps"] count the rows and steps of such calls.  Any other value, a live
        call (an index on a live call is still out) or an attn_fp8 engine is a ValueError naming `rows` / `attn_fp8`, before anything is
        launched."""
        dev, dt = self.device, self.dtype
        if rows not in self.ROWS:
            raise ValueError(f"rows={rows!r}: \"all\" (every loop step runs the [uncond | cond] rows of every person) or \"needed\" (a step "
                             "runs only the rows its persons need)")
        if rows == "needed" and not isinstance(cloth, GarmentCache):
            raise ValueError("rows=\"needed\" reads the garments through an index table, and an index on a live call is still out: pass a "
                             "GarmentCache as `cloth=`")
        if rows == "needed" and self.unet.attn_fp8:
            raise ValueError("rows=\"needed\": attn_fp8 mismatch (the row plan is not run by an attn_fp8 engine)")
        self._release_streamed()
        f32 = lambda t: t.to(dev, torch.float32).contiguous()
        gcache = cloth if isinstance(cloth, GarmentCache) else None
        if gcache is not None and gcache.features:
            self._refuse_features_fp8("prepare(cloth=<feature cache>)")
        if garment_index is not None and gcache is None:
            raise ValueError("garment_index names garments of a GarmentCache: pass one as `cloth=` (a live call encodes one garment per person)")
        gindex = None
        if gcache is not None and gcache.sizes is not None and garment_index is None:
            raise ValueError("a GarmentCache with `sizes` holds garments of several sizes: pass garment_index (person i wears garment "
                             "garment_index[i]; the i % G rule of a plain cache does not apply)")
        g_b, phi_b, guided, skip = self._guidance(image.shape[0], guidance_scale, guidance_rescale, uncond)
        s_b, n_b = self._person_steps(image.shape[0], strength, num_inference_steps)
        s_min = strength if s_b is None else min(s_b)
        if s_b is not None:                                  # the loop runs the longest list: every person's is a suffix of it
            strength = max(s_b)
        plans = None
        if rows == "needed":                                 # the row plan, or None: nothing to skip -- the state the call is today
            plans = self._row_plans(image.shape[0], n_b, g_b, len(self._timesteps(scheduler, num_inference_steps, strength)[1]))
            if plans is None and max(g_b) <= 1:              # nobody with guidance, nobody dormant: the conditional branch alone
                skip = True
            guided = guided or skip or plans is not None
        if gcache is not None:
            gidx = gcache.check(timesteps=self._timesteps(scheduler, num_inference_steps, strength)[1],
                                h=(height or image.shape[-2]) // 8, w=(width or image.shape[-1]) // 8, dtype=dt, attn_fp8=self.unet.attn_fp8,
                                f8_exp=self.unet.f8_exp, weights_id=self.weights_identity(), persons=image.shape[0], garment_index=garment_index)
            if garment_index is not None:
                gidx, gindex = gidx
            elif plans is not None:                          # a row state reads every garment through a table: the i % G rule, written out
                gindex = [i % gcache.G for i in range(image.shape[0])]
            if gcache.host_resident:
                self._check_host_cache(gcache)
        image, mask_image, pose_img = f32(image), f32(mask_image), f32(pose_img)
        cloth = f32(cloth) if gcache is None else None
        B = image.shape[0]
        H = height or image.shape[-2]
        W = width or image.shape[-1]
        h, w = H // 8, W // 8
        gh, gw = self._garment_latent_size(cloth) if gcache is None else (gcache.gh, gcache.gw)
        # any H x W divisible by 8 (the reference's own check, tryon_pipeline.py check_inputs): odd latent levels go through `upsample_size`
        # (unet.py: _conv3 out_hw), token counts that are not a multiple of 16 are padded inside each Transformer2DModel (unet.py: _transformer)
        if H % 8 or W % 8:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {H} and {W}.")
        start_is_given = bool(noise.get("latents_given"))    # the reference's `latents=` argument: used as the start as they are (:880-882)
        if s_min < 1.0 and noise.get("image") is None and not start_is_given:
            raise ValueError("strength < 1 starts from add_noise(encode(image)): pass the posterior draw of the init-image encode as "
                             "noise['image'] (the reference's first random draw, tryon_pipeline.py:883-889), or set noise['latents_given'] "
                             "when noise['latents'] already is the start (the reference's `latents=` argument)")
        sched, timesteps = self._timesteps(scheduler, num_inference_steps, strength)
        lay1 = skip and plans is None                        # (a row state builds the full [uncond | cond] layout and gathers from it)
        if lay1:                                             # the conditional branch alone: nothing unconditional is read
            if ip_hidden_states is not None and ip_hidden_states.shape[0] == 2 * B:
                ip_hidden_states = ip_hidden_states[B:]
            if image_embeds is not None and image_embeds.shape[0] == 2 * B:
                image_embeds = image_embeds[B:]
        elif max(g_b) <= 1:                                                                # no CFG: see the docstring
            guidance_scale = 1.0
            if negative_prompt_embeds is None:
                negative_prompt_embeds = torch.zeros_like(prompt_embeds)
            if negative_pooled_prompt_embeds is None:
                negative_pooled_prompt_embeds = torch.zeros_like(pooled_prompt_embeds)
            if ip_hidden_states is not None and ip_hidden_states.shape[0] == B:
                ip_hidden_states = torch.cat([torch.zeros_like(ip_hidden_states), ip_hidden_states])
            if image_embeds is not None and image_embeds.shape[0] == B:
                image_embeds = torch.cat([torch.zeros_like(image_embeds), image_embeds])

        init_image = 2.0 * image - 1.0                                                     # preprocess :1588-1591
        mask = (mask_image >= 0.5).float()                                                 # mask_processor :1593-1595
        masked_image = init_image * (mask < 0.5)                                           # :1602
        if s_b is not None:
            latents = self._person_starts(sched, timesteps, s_b, n_b, noise, start_is_given,
                                          init_image if image_dtype is None else init_image.to(image_dtype).float())
        elif strength == 1.0 or start_is_given:
            latents = f32(noise["latents"]) * sched.init_noise_sigma                       # :889-893
        else:                                                                              # image + noise start (:883-891)
            src = init_image if image_dtype is None else init_image.to(image_dtype).float()    # prepare_latents casts the image (:884)
            ab = float(sched.alphas_cumprod[int(timesteps[0])])
            latents = ab ** 0.5 * self.vae.encode_sample(src, f32(noise["image"])) + (1.0 - ab) ** 0.5 * f32(noise["latents"])
        mask_l = torch.nn.functional.interpolate(mask, size=(h, w))                        # :939-941
        # the three VAE encodes of the call (:964 masked image, :1644-1647 pose, :1654 cloth) as ONE encoder pass over 3B images: per
        # image the arithmetic is unchanged (GroupNorm / attention are per image), the convolution GEMMs see 3x the rows and the
        # launch count of the encoder is paid once
        if gcache is None and tuple(cloth.shape[-2:]) == (H, W):
            enc = self.vae.encode_sample(torch.cat([masked_image, pose_img, cloth]),
                                         torch.cat([f32(noise["masked"]), f32(noise["pose"]), f32(noise["cloth"])]))
            masked_lat, pose_lat, cloth_lat = enc[:B], enc[B:2 * B], enc[2 * B:]
        else:                                                # the pass is over 2B images: the garment is already encoded (a cache) ...
            enc = self.vae.encode_sample(torch.cat([masked_image, pose_img]), torch.cat([f32(noise["masked"]), f32(noise["pose"])]))
            masked_lat, pose_lat, cloth_lat = enc[:B], enc[B:], None
            if gcache is None:                               # ... or has a size of its own, and a pass of its own
                cloth_lat = self.vae.encode_sample(cloth, f32(noise["cloth"]))
        # step-invariant 9 conditioning channels of the 13-channel input, NHWC, both CFG halves (:955,977,1649-1652,1777)
        cond = torch.cat([mask_l, masked_lat, pose_lat], dim=1).permute(0, 2, 3, 1).reshape(B, h * w, 9)
        nrows = B if lay1 else 2 * B                         # TryonNet rows: [uncond | cond], or the conditional branch alone
        cond = (cond if lay1 or plans is not None else torch.cat([cond, cond], dim=0)).to(dt).contiguous()   # (a row state: one row per person)

        if lay1:
            pe, add_text = prompt_embeds.to(dev), pooled_prompt_embeds.to(dev)
        else:
            pe = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0).to(dev)             # :1710
            add_text = torch.cat([negative_pooled_prompt_embeds, pooled_prompt_embeds], dim=0).to(dev)   # :1711
        time_ids = torch.tensor([[H, W, 0, 0, H, W]], dtype=torch.float32, device=dev).repeat(nrows, 1)  # :1681-1713
        if image_embeds is None:
            image_embeds = self.resampler(ip_hidden_states.to(dev))                        # :1726 (encoder_hid_proj)
        ctx_t = self.unet.encode_context(pe, image_embeds)
        temb_t = self.unet.time_embeddings(timesteps, nrows, dict(text_embeds=add_text, time_ids=time_ids))
        if gcache is None:
            # GarmentNet over consecutive timesteps per batch, blocks of 1, 2, 4, k, k, ... timesteps
            garm = dict(self._garment_inputs(cloth_lat, text_embeds_cloth, timesteps, B), gcache=None, gidx=None, garment_persons=None,
                        gindex=None, gix=None, gnk=None)
        else:                                                # the same blocks drive the loop; their garment side is a read of the cache
            k, blocks = self._block_schedule(len(timesteps))
            if gcache.sizes is not None:                     # [features][2B]: the real tokens of person b % B's garment, in both CFG halves
                per = [self.unet.feature_tokens(*sz) for sz in gcache.garment_sizes(gindex)]   # (uncond="skip": [features][B])
                gnk = torch.tensor([[p[f] for p in per] * (nrows // B) for f in range(len(per[0]))], dtype=torch.int32, device=dev)
            garm = dict(cloth=None, ctx_g=None, temb_g=None, k=k, blocks=blocks, temb_gk=None, cloth_k=None, ctx_gk=None,
                        gcache=gcache, gidx=gidx, garment_persons=B, gindex=gindex,
                        # the table the kernels read: person -> garment of the cache (a graph state keeps its own: person -> set slot)
                        gix=torch.tensor(gindex, dtype=torch.int32, device=dev) if gindex is not None else None,
                        # the second table, on a cache with sizes only: per garment feature the key count of every batch
                        gnk=gnk if gcache.sizes is not None else None)
        if s_b is not None and plans is None:                # [steps][3 + 3B]: the guided row and who takes the step; the same scratch
            coef = torch.tensor(sched.person_coef_table(timesteps, g_b, phi_b, n_b), dtype=torch.float32, device=dev)
            work = torch.empty(ops.guided_step_work_floats(B, h * w), dtype=torch.float32, device=dev) if not skip else None
        elif guided:                                         # [steps][3 + 2B], and the statistics scratch of idmvton_guided_step
            coef = torch.tensor(sched.guided_coef_table(timesteps, g_b, phi_b), dtype=torch.float32, device=dev)
            work = torch.empty(ops.guided_step_work_floats(B, h * w), dtype=torch.float32, device=dev) if not lay1 else None
        else:
            coef, work = torch.tensor(sched.coef_table(timesteps, guidance_scale), dtype=torch.float32, device=dev), None
        steps_noise = f32(noise["steps"]) if noise.get("steps") is not None and scheduler == "ddpm" else None
        return dict(B=B, h=h, w=w, gh=gh, gw=gw, timesteps=timesteps, latents=latents.contiguous(), cond=cond,
                    ctx_t=ctx_t, temb_t=temb_t, coef=coef, steps_noise=steps_noise, **garm,
                    guided=guided, branches=1 if lay1 else 2, work=work, **(dict(person=True, n_active=n_b) if s_b is not None and plans is None else {}),
                    **(dict(rows=self._bind_rows(plans, ctx_t, temb_t, garm)) if plans is not None else {}),
                    x_in=torch.empty(max(p["R"] for p in plans[1]) if plans is not None else nrows, h * w, self.unet.cin_pad, dtype=dt, device=dev),
                    trace=dict(masked_lat=masked_lat, pose_lat=pose_lat, cloth_lat=cloth_lat, image_embeds=image_embeds))

    def _bind_rows(self, plans, ctx_t, temb_t, garm):
        """st["rows"] of a row state: _row_plans' result with what each plan's steps read, gathered from the full [uncond B | cond B]
        layout (so every value has the bits of the rows="all" call): per plan the device tables row_person[R] and {urow | crow}[2B], the
        context K rows / V^T entries of full_rows for every attn2, the key-count columns of full_rows (a cache with sizes) and the active
        persons' garment index; per step the time embeddings of its plan's rows."""
        dev = self.device
        index, plans = plans
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        bound = []
        for p in plans:
            fr, act = torch.tensor(p["full_rows"], device=dev), torch.tensor(p["persons"], device=dev)
            ctx = {**ctx_t, "B": p["R"], "kv": {}}
            for name, ent in ctx_t["kv"].items():            # K [2B * r][C] -> the rows' r-row runs; V^T [2B][C][r] -> the rows' entries
                ctx["kv"][name] = {kind: (t.view(ctx_t["B"], -1, t.shape[-1])[fr].reshape(-1, t.shape[-1]) if kind in ("kt", "ki") else t[fr]).contiguous()
                                   for kind, t in ent.items()}
            bound.append(dict(p, persons_t=act, row_person_t=i32(p["row_person"]), table=i32(p["urow"] + p["crow"]), ctx=ctx,
                              gix=garm["gix"][act].contiguous(), gnk=garm["gnk"][:, fr].contiguous() if garm["gnk"] is not None else None))
        return dict(step=index, plans=bound, temb=[temb_t[j][torch.tensor(plans[pi]["full_rows"], device=dev)] for j, pi in enumerate(index)])

    def _person_starts(self, sched, timesteps, s_b, n_b, noise, start_is_given, src):
        """The start latents of a call with a strength per person: person i's row is what the scalar call at s_i forms for it -- the noise
        as it is at s_i == 1 (or when the latents are given), else add_noise(encode(image_i), noise_i, its own first timestep), with the scalar
        path's Python-float arithmetic, one alpha-bar per person.  The image encode is the scalar call's: one pass over the whole batch."""
        f32 = lambda t: t.to(self.device, torch.float32).contiguous()
        nz = f32(noise["latents"])
        if start_is_given or min(s_b) == 1.0:
            return nz * sched.init_noise_sigma                                             # :889-893
        enc = self.vae.encode_sample(src, f32(noise["image"]))
        rows = []
        for i, (s, n_i) in enumerate(zip(s_b, n_b)):
            if s == 1.0:
                rows.append(nz[i:i + 1] * sched.init_noise_sigma)
            else:                                                                          # image + noise start (:883-891)
                ab = float(sched.alphas_cumprod[int(timesteps[len(timesteps) - n_i])])
                rows.append(ab ** 0.5 * enc[i:i + 1] + (1.0 - ab) ** 0.5 * nz[i:i + 1])
        return torch.cat(rows)

    # ---- blocks: one GarmentNet batch over k timesteps + the k TryonNet steps that consume it ------------------------------
    # The GarmentNet batch of block b+1 -- and the attn1 K / V^T projections of its features with TryonNet's weights -- can run on a
    # second HIP stream while TryonNet runs the steps of block b (drive_blocks).  Two feature sets alternate; there is no other coupling.
    # `st` below is a call's state (prepare) or a persistent graph state (_graph_state): both carry the keys these two read.
    def _garment_feats(self, st, temb_gk, feats_buf, c=None):
        """One GarmentNet batch over c timesteps -> its 70 features, written into feats_buf."""
        B, h, w = st["B"], st["gh"], st["gw"]                # GarmentNet runs at the garment's own latent size
        c = st["k"] if c is None else c                      # timesteps in this batch (the set's buffers hold up to st["k"])
        self.stats["garment_batches"] += 1
        return self.unet_encoder.forward(st["cloth_k"][:c * B], temb_gk[:c * B], st["ctx_gk"], c * B, h, w, feats_buf=feats_buf)[1]   # :1787

    def _garment_side(self, st, temb_gk, fset, c=None):
        self.unet.project_garment_kv(self._garment_feats(st, temb_gk, fset["feats"], c), out=fset["kv"])

    def _count_step(self, st, plan=None):
        """The one place a loop step of a call is counted, by the `step` of either execution form (a launch or a replay; warm-ups and
        captures are not steps of a call).  A kind that has no counter lists none in stats."""
        kind = self._kind(st)
        if kind == "person":
            self.stats["person_steps"] += 1
        elif kind == "rows":
            self.stats["tryon_rows"] += plan["R"]
            self.stats["row_steps"] += 1

    def _tryon_main(self, st, temb_t, coef, noise, kv_j, plan=None):
        B, h, w, kind = st["B"], st["h"], st["w"], self._kind(st)
        if kind == "rows":                                   # the step's plan: R = u + a rows, the last a of them conditional
            R = plan["R"]
            x = ops.pack_rows(st["latents"], st["cond"], st["x_in"][:R], plan["row_person_t"])
            eps, _ = self.unet.forward(x, temb_t, plan["ctx"], R, h, w, garment_kv=kv_j, garment_persons=plan["a"], garment_hw=(st["gh"], st["gw"]),
                                       garment_index=plan["gix"], garment_nk=plan["gnk"])
            ops.row_step(eps, st["latents"], noise, coef, st["work"], plan["table"])
            return eps
        branches = st.get("branches", 2)                     # 1: uncond="skip", the conditional rows alone (garment segment from batch 0 on)
        (ops.pack_input if branches == 2 else ops.pack_input_cond)(st["latents"], st["cond"], st["x_in"])   # :1769,1777
        # garment_persons: None = one garment entry per conditional batch (unet.forward's default); B on a GarmentCache call, where kv_j
        # holds G garments for the B persons (a shared segment when G < B)
        eps, _ = self.unet.forward(st["x_in"], temb_t, st["ctx_t"], branches * B, h, w, garment_kv=kv_j, garment_persons=st["garment_persons"],
                                   garment_hw=(st["gh"], st["gw"]), garment_index=st.get("gix"), garment_nk=st.get("gnk"))   # :1796-1808
        if kind == "person":                                 # a strength per person: the guided step for those the coef row calls active
            ops.person_step(eps, st["latents"], noise, coef, st["work"], branches)
        elif kind == "guided":                               # per-person guidance / rescale, or e = t of the conditional branch alone
            ops.guided_step(eps, st["latents"], noise, coef, st["work"], branches)         # :1814-1823
        else:
            ops.cfg_step(eps, st["latents"], noise, coef)                                  # :1814-1823
        return eps

    def _discover_set_shapes(self, st):
        """-> (feature shapes, (K, V^T) shapes) of a GarmentNet batch over k timesteps, learnt once per (B, gh, gw, k) by running one (its
        outputs are dropped; not counted in stats)."""
        B, h, w, k = st["B"], st["gh"], st["gw"], st["k"]
        key = self._set_key(st)
        if key not in self._set_shapes:
            _, feats = self.unet_encoder.forward(st["cloth_k"], st["temb_gk"][0], st["ctx_gk"], k * B, h, w)
            kv = self.unet.project_garment_kv(feats)         # (dtype uint8 = e4m3: attn_fp8)
            self._set_shapes[key] = ([tuple(f.shape) for f in feats], kv_shapes(kv))
        return self._set_shapes[key]

    def _alloc_set(self, feat_shapes, shapes, n, k, G):
        """A persistent {features, (K, V^T)} set for up to k timesteps of G garments + per-timestep views of its K / V^T, uninitialised;
        `shapes` are those of a (K, V^T) list that holds n timesteps."""
        kv = alloc_kv(shapes, n, k, self.device)
        return dict(feats=[torch.empty(sh, dtype=self.dtype, device=self.device) for sh in feat_shapes], kv=kv,
                    step=[timestep_run(kv, k, G, j) for j in range(k)])

    def _new_set(self, st):
        """The set of a live call: 70 features and 70 (K, V^T) of a GarmentNet batch over st["k"] timesteps.  A plain allocation:
        _garment_side fills it."""
        fs, ks = self._discover_set_shapes(st)
        return self._alloc_set(fs, ks, st["k"], st["k"], st["B"])

    def _fill_set(self, st, fset, s0, c):
        """Steps s0 .. s0 + c - 1 of the call: their cached K / V^T -> the first c timestep slots of a persistent set (current stream).  The
        call's timesteps are consecutive cache entries unless the scheduler says otherwise: one copy per tensor then, else one per timestep.
        With garment_index: the U distinct garments the call uses, in first-use order, -> slots 0 .. U - 1 of each timestep slot of a P-slot
        set (the state's table maps persons to those slots; no slot beyond U is ever indexed): per timestep one copy per tensor and run of
        consecutive garments, so the bytes moved scale with what the call uses, not with the pool."""
        gc, idx = st["gcache"], st["gidx"][s0:s0 + c]
        self.stats["garment_set_copies"] += 1
        if st["gindex"] is not None:
            n, P = len(gc.timesteps), st["B"]
            runs = index_runs(list(dict.fromkeys(st["gindex"])))
            for j, i in enumerate(idx):
                for d0, g0, cc in runs:
                    for d, s in zip(slot_run(fset["kv"], st["k"], P, j, d0, cc), slot_run(gc.kv, n, gc.G, i, g0, cc)):
                        for dt, src in zip(d, s):
                            dt.copy_(src)
            return
        runs = [(0, idx[0], c)] if idx == list(range(idx[0], idx[0] + c)) else [(j, i, 1) for j, i in enumerate(idx)]
        for j0, i0, cc in runs:
            for d, s in zip(timestep_run(fset["kv"], st["k"], gc.G, j0, cc), gc.run(i0, cc)):
                for dt, src in zip(d, s):
                    dt.copy_(src)

    @staticmethod
    def _cache_set_shapes(st):
        """-> (slots, shapes) of a persistent set for a call on a GarmentCache: one slot per garment of the cache -- or, with garment_index,
        one per PERSON, whatever the pool holds --, (K, V^T) shapes of a list holding the cache's n timesteps, in the engine's 16-bit dtype
        (a packed cache's bytes are widened on the way in).  A feature cache gives the shapes a K / V^T cache of the same garments gives,
        derived from F's: the sets hold what the block's projection writes."""
        gc = st["gcache"]
        slots = gc.G if st["gindex"] is None else st["B"]
        if isinstance(gc, ShelvedGarmentCache):              # no tensor list: the slot's shapes, what a slotted cache of that slot size has
            n = len(gc.timesteps)                            # (K / V^T and feature parts alike: the sets hold what the projection writes)
            return slots, [((n * slots * a[0], a[1]), (n * slots, b[0], b[1]), gc.dtype) for a, b in gc.slot_shapes]
        if gc.features:
            return slots, TryonEngine._feature_kv_shapes(gc, slots)
        dt = lambda d: gc.dtype if gc.packed else d
        return slots, [((a[0] // gc.G * slots,) + a[1:], (b[0] // gc.G * slots,) + b[1:], dt(d)) for a, b, d in kv_shapes(gc.kv)]

    def _check_host_cache(self, gc):
        """The conditions under which a host-resident cache can be streamed; ValueError naming the field otherwise.  A pageable address must
        never reach a descriptor (the GPU would fault on it), so the refusal is here, before any table is built."""
        if self.unet.attn_fp8:
            raise ValueError("host-resident GarmentCache attn_fp8 mismatch: an attn_fp8 engine does not stream a cache from host memory "
                             "(move it with .to(device))")
        if isinstance(gc, ShelvedGarmentCache):              # the host-resident cache WITH sizes: every part held to the same conditions
            for part in gc.parts:
                self._check_host_cache(part)
            return
        if gc.sizes is not None:
            raise ValueError("host-resident GarmentCache sizes mismatch: a cache with `sizes` (slotted / mixed_sizes) is not streamed from host "
                             "memory (move it with .to(device))")
        if not all(t.is_pinned() for e in gc.kv for t in e):
            raise ValueError("host-resident GarmentCache kv mismatch: the tensors are pageable host memory; the device reads page-locked memory "
                             "only -- make the cache with .to(\"cpu\", pin_memory=True) or GarmentPool(resident=\"host\")")
        if gc.packed and not gc.exps.is_pinned():
            raise ValueError("host-resident GarmentCache exps mismatch: the exponents are pageable host memory; the device reads page-locked "
                             "memory only -- make the cache with .to(\"cpu\", pin_memory=True) or GarmentPool(resident=\"host\")")

    def _release_streamed(self):
        """Drop the engine's references to host-resident caches whose last queued fill has completed (an event that was never recorded counts
        as passed).  Called by every `prepare`, `decode` and `_cached_fill`, and after a graph state's warm-up: the engine keeps a streamed
        cache alive from its first fill until the first of those calls after its last fill has finished -- not beyond the next call."""
        self._streaming = [h for h in self._streaming if not h[1].query()]

    HOST_TRANSPORTS = ("kernel", "copy")

    @classmethod
    def _check_host_transport(cls, host_transport):
        if host_transport not in cls.HOST_TRANSPORTS:
            raise ValueError(f"host_transport={host_transport!r}: \"kernel\" (a kernel reads the page-locked cache: idmvton_kv_stream / idmvton_kv_fill) "
                             "or \"copy\" (the copy engines fill a staging arena, idmvton_kv_place places it)")

    def _cached_fill(self, st, sets, blocks=None):
        """-> garment(bi, p) of a call on a GarmentCache: block bi's cache entries -> the first timestep slots of sets[p], on the current
        stream.  The gather is always _fill_set's -- entries by value, consecutive or not; with garment_index the U distinct garments in
        first-use order into slots 0 .. U - 1 of P-slot sets --; what the cache is decides how it is carried out:
          16-bit, on the device      _fill_set itself: copies.
          packed, on the device      ONE idmvton_kv_unpack launch widens the block's bytes.
          host-resident              ONE idmvton_kv_stream launch (shelved: idmvton_kv_fill, which also writes the zero V^T tail behind each
                                     compact garment) reads page-locked host memory, widening e4m3 bytes or copying 16-bit values.
          host-resident, st["host_transport"] == "copy"
                                     the block's source bytes go into a block-sized STAGING ARENA in HBM by copy_(non_blocking=True) -- the
                                     copy engines, no kernel reads the host link -- and ONE idmvton_kv_place launch places them
                                     (garment_cache.staged_plan).  Block b + 1's copies follow block b's launch in stream order, so one arena
                                     serves both sets; it belongs to the engine, one per call shape (the sets' key, the source's storage, U),
                                     k x the used garments' source bytes per timestep, and a shelved call with larger garments replaces it.
                                     A packed source's exponents go to a small device tensor once per call, here.
        The launched forms are descriptors (garment_cache.kv_records), one table for every (set, step): cache, set, arena and exponent
        addresses are all stable, so table and prefix tables are built and uploaded ONCE, here, with one idmvton_host_device_ptr per host
        tensor, and a block is a slice.  `blocks`: build for these block numbers only (the warm-up; the arena's table covers k timesteps per
        set whatever the blocks, a block of c being a prefix).  Launches and copies read a host-resident cache by raw address: it stays
        referenced by the engine until the event behind the last one has passed (_release_streamed).
        A FEATURE cache (gc.features) holds GarmentNet's features F, not their K / V^T: every form above then moves the block's F entries into
        the first c * S slots of a feature STAGING list of set p -- a live set's `feats` shapes, allocated on first use and kept by the set --
        in place of the set's K / V^T, and ONE project_garment_kv(staging, out=sets[p]["kv"]) follows it on the same stream: the launches
        an uncached call makes behind its GarmentNet batch.  Same tables, same records (F is K-shaped: kv_records), same transports, same sets
        and graph states.  A device-resident 16-bit block of consecutive entries without an index is projected from the cache's own views,
        with no copy.  Slots no person reads are projected from whatever the staging list holds.
        A SHELVED feature cache (ShelvedGarmentCache of feature parts) is both at once: idmvton_kv_fill / idmvton_kv_place puts each compact
        F into the front of its staging slot and writes the zero ROWS behind it (kv_records), and the projection -- at slot size whatever
        the garments' sizes -- makes zero K rows and the zero V^T tail of them: to_k / to_v have no bias.  The sets, tables and graph states
        are those of the K / V^T shelf call at the same slot size."""
        gc, k, B = st["gcache"], st["k"], st["blocks"]
        S = gc.G if st["gindex"] is None else st["B"]
        dsts, project = [fs["kv"] for fs in sets], lambda bi, p, feats=None: None
        if gc.features:
            n = len(gc.timesteps)
            # (N_f, C_f) of a staging slot: a shelved cache has no tensor list -- the slot's K shape, whatever its compact parts hold
            fshapes = [a for a, _ in gc.slot_shapes] if isinstance(gc, ShelvedGarmentCache) else [(f.shape[0] // (n * gc.G), f.shape[1]) for f, in gc.kv]
            for fs in sets:
                if not fs["feats"]:
                    fs["feats"] = [torch.empty(k * S, N, Cc, dtype=self.dtype, device=self.device) for N, Cc in fshapes]
            dsts = [[(f.view(-1, f.shape[-1]),) for f in fs["feats"]] for fs in sets]

            def project(bi, p, feats=None):
                self.stats["garment_projections"] += 1
                self.unet.project_garment_kv([f[:B[bi][1] * S] for f in sets[p]["feats"]] if feats is None else feats, out=sets[p]["kv"])
        if not (gc.packed or gc.host_resident):
            def garment(bi, p):
                s0, c = B[bi]
                idx = st["gidx"][s0:s0 + c]
                if gc.features and st["gindex"] is None and idx == list(range(idx[0], idx[0] + c)):
                    return project(bi, p, self._feature_views(gc.run(idx[0], c), c * S))
                self._fill_set(st, dict(kv=dsts[p]), s0, c)
                project(bi, p)
            return garment
        garments = list(range(gc.G)) if st["gindex"] is None else list(dict.fromkeys(st["gindex"]))
        staged = gc.host_resident and st.get("host_transport") == "copy"
        built = [bi for bi in range(len(B)) if staged or blocks is None or bi in blocks]
        if staged:
            key = self._set_key(st) + (torch.uint8 if gc.packed else gc.dtype, len(garments), gc.features)
            plan = staged_plan(gc, st["gindex"], k, S, dsts, self.device, *self._arenas.get(key, (None, None)))
            self._arenas[key] = (plan["arena"], plan["exps"])
            rec, per, rows, row = plan["rec"], plan["per"], k, dict.fromkeys(built, 0)
            copies = [plan["copies"](st["gidx"][s0:s0 + c]) for s0, c in B]
        else:
            steps = [(B[bi][0] + j, j) for bi in built for j in range(B[bi][1])]
            first = {i: at for at, (i, _) in enumerate(steps)}
            rows, row = len(steps), {bi: first[B[bi][0]] for bi in built}   # block -> the place of its first step in a set's part of the table
            rec, per = kv_records(cache_sources(gc, garments), dsts, k, S, [st["gidx"][i] for i, _ in steps], [j for _, j in steps],
                                  ops.stream_address if gc.host_resident else None)   # (records per step, even: every slice starts 16-byte aligned)
        at = {(p, bi): ((p * rows + row[bi]) * per, B[bi][1] * per) for p in range(len(sets)) for bi in built}
        if not gc.host_resident:
            table = ops.KvUnpackTable(rec, self.device)

            def garment(bi, p):
                self.stats["garment_set_copies"] += 1
                table.launch(self.dtype, *at[(p, bi)])
                project(bi, p)
            return garment
        slices = sorted(set(at.values()))
        cls = ops.KvPlaceTable if staged else ops.KvFillTable if isinstance(gc, ShelvedGarmentCache) else ops.KvStreamTable
        table = cls(rec, self.device, ops.ffi.KVS_WIDEN_E4M3 if gc.packed else ops.ffi.KVS_COPY, slices)
        self._release_streamed()
        hold = [gc, torch.cuda.Event()]
        self._streaming.append(hold)
        for dst, src in plan["exps_copies"] if staged else ():
            dst.copy_(src, non_blocking=True)

        def garment(bi, p):
            if staged:
                for dst, src in copies[bi]:
                    dst.copy_(src, non_blocking=True)
                self.stats["garment_stage_copies"] += len(copies[bi])
            self.stats["garment_stage_launches" if staged else "garment_stream_launches"] += 1
            table.launch(self.dtype, slices.index(at[(p, bi)]))
            hold[1].record()                                 # the call's last fill so far: until it has passed, `hold` keeps the cache alive
            project(bi, p)
        return garment

    def _slot_table(self, st):
        """Graph forms with garment_index: person -> slot of the persistent sets, where _fill_set puts the call's distinct garments in
        first-use order ([7, 7, 3, 9] -> [0, 0, 1, 2]); None without an index."""
        if st["gindex"] is None:
            return None
        slot = {g: u for u, g in enumerate(dict.fromkeys(st["gindex"]))}
        return torch.tensor([slot[g] for g in st["gindex"]], dtype=torch.int32, device=self.device)

    def _noise(self, st, i):
        return st["steps_noise"][i] if st["steps_noise"] is not None else None

    # ---- the execution forms: each hands drive_blocks its two callables ----------------------------------------------------
    # -> (garment(bi, p), step(i, j, p), the latents the steps update, (side stream, ready, free) | None = serial order).
    # `live` (denoise: GarmentNet runs in this call / its K, V^T are read from st["gcache"]) picks one row of each form's table.
    def _eager_form(self, st, live, overlap):
        blocks = st["blocks"]
        if live:
            sets = [self._new_set(st) for _ in range(2 if overlap else 1)]
            garment = lambda bi, p: self._garment_side(st, st["temb_gk"][bi], sets[p], blocks[bi][1])
            kv = lambda i, j, p: sets[p]["step"][j]
        elif st["gcache"].packed or st["gcache"].host_resident or st["gcache"].features:
            # e4m3 bytes, host memory, or features still to be projected: TryonNet reads 16-bit sets on the device, as the graph forms do
            # (one, or two to overlap)
            slots, shapes = self._cache_set_shapes(st)
            sets = [self._alloc_set((), shapes, len(st["gcache"].timesteps), st["k"], slots) for _ in range(2 if overlap else 1)]
            garment = self._cached_fill(st, sets)
            st = dict(st, gix=self._slot_table(st))          # with garment_index: person -> set slot (the same tensors otherwise)
            if st.get("rows"):                               # (a row state: each plan's active persons -> set slots)
                st["rows"] = dict(st["rows"], plans=[dict(p, gix=st["gix"][p["persons_t"]].contiguous()) for p in st["rows"]["plans"]])
            kv = lambda i, j, p: sets[p]["step"][j]
        else:                                                # nothing to launch, so nothing to overlap: TryonNet reads the cache's own views
            overlap = False
            garment = lambda bi, p: None
            kv = lambda i, j, p: st["gcache"].step(st["gidx"][i])
        rw = st.get("rows")

        def step(i, j, p):
            plan = rw["plans"][rw["step"][i]] if rw else None                              # a row state: the step is handed its plan
            self._count_step(st, plan)
            self._tryon_main(st, (rw["temb"] if rw else st["temb_t"])[i], st["coef"][i], self._noise(st, i), kv(i, j, p), plan)
        if not overlap:
            return garment, step, st["latents"], None
        if self._side is None:
            self._side = torch.cuda.Stream()
        ready, free = [torch.cuda.Event(), torch.cuda.Event()], [torch.cuda.Event(), torch.cuda.Event()]
        return garment, step, st["latents"], (self._side, ready, free)

    def _graph_state(self, st, live):
        """Persistent buffers + captured graphs for one shape; it owns exactly what a captured graph reads or writes (latents, cond, x_in, the
        ctx_t K / V^T and, live, cloth_k and the ctx_gk K / V^T: the first call's tensors, adopted; the two sets; tt / cf / nz / tgk) and
        the scalars B, h, w, gh, gw, k, garment_persons -- nothing else of a call, so no GarmentCache and no time-embedding table stays alive here.
        The graphs are SMALL: ('garm', p, c) = the GarmentNet batch into feature set p, ('tryon', p, j) = one TryonNet step on timestep
        slice j of set p (2 + 2k graphs, captured on first use).  The loop replays them like the eager form launches kernels -- GarmentNet
        graphs on the side stream, TryonNet graphs on the main stream, two events per set -- so the overlap form has no fork/join inside a
        graph and a replay never queues more than one step.  (One graph per 6-step block, GarmentNet as a parallel branch, measured 1.2 %
        slower than eager launch; this form matches it.)  On a GarmentCache call the sets hold cache entries and there are no 'garm' graphs.
        Captures use capture_error_mode="thread_local": with torch.distributed / RCCL initialised a watchdog thread polls events,
        which the default global mode would treat as a capture violation."""
        has_noise = st["steps_noise"] is not None
        key = self._graph_key(st, live)                      # garment size included: calls with different garment sizes share nothing here
        if key in self._graphs:
            return self._graphs[key]
        rows = st["rows"] if self._kind(st) == "rows" else None
        G = {name: st[name] for name in ("B", "h", "w", "gh", "gw", "k", "garment_persons", "latents", "cond", "x_in") + (() if rows else ("ctx_t",))}
        if rows:
            # a ROW state serves every plan of every call of its shape: x_in and tt hold 2B rows and a step uses their first R; what a
            # plan's captures read besides -- context, index, key counts, the two plan tables -- lives in persistent buffers per (R, a),
            # made on first use and copied per call (_state_rows)
            G.update(x_in=torch.empty(2 * st["B"], *st["x_in"].shape[1:], dtype=self.dtype, device=self.device), rows={})
        # guided: the scratch of idmvton_guided_step, persistent like gix / gnk (the captures hold its pointer; its contents carry nothing
        # from one step to the next, so the first call's buffer is adopted and never copied)
        G.update(guided=st.get("guided", False), branches=st.get("branches", 2), work=st.get("work"), person=self._kind(st) == "person")
        # indexed: the table person -> set slot, a persistent buffer whose pointer the captured graphs hold; its contents are copied per call
        G["gix"] = self._slot_table(st) if not rows else None
        # ragged: the key-count table, persistent in the same way (the sets copy whole slots, so it is the call's own table)
        G["gnk"] = st["gnk"].clone() if st.get("gnk") is not None and not rows else None
        G.update(tt=st["temb_t"][0].clone(), cf=st["coef"][0].clone(), nz=st["steps_noise"][0].clone() if has_noise else None, graphs={},
                 side=torch.cuda.Stream(), ready=[torch.cuda.Event(), torch.cuda.Event()], free=[torch.cuda.Event(), torch.cuda.Event()],
                 # graphs that replay one after another on ONE stream may share a memory pool: all TryonNet graphs (main stream), all
                 # GarmentNet graphs (side stream)
                 pools=dict(tryon=torch.cuda.graph_pool_handle(), garm=torch.cuda.graph_pool_handle()))
        saved = st["latents"].clone()
        warm = torch.cuda.Stream()
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):                                # warm-up off the default stream (allocator, lazy init)
            if live:
                G.update(cloth_k=st["cloth_k"], ctx_gk=st["ctx_gk"], tgk=st["temb_gk"][0].clone())
                G["sets"] = [self._new_set(st), self._new_set(st)]
                self._garment_side(G, G["tgk"], G["sets"][0])
            else:                                            # the first block's fill stands in for a warm-up batch
                gc = st["gcache"]
                slots, shapes = self._cache_set_shapes(st)   # (with an index: one slot per person, whatever the pool holds)
                G["sets"] = [self._alloc_set((), shapes, len(gc.timesteps), st["k"], slots) for _ in range(2)]
                self._cached_fill(st, G["sets"][:1], blocks=(0,))(0, 0)   # (a table of block 0 alone: complete before the synchronize below)
                if gc.features:                              # garment_projections counts the blocks of calls: not the warm-up's
                    self.stats["garment_projections"] -= 1
            self._state_step(G, 0, 0, self._state_rows(G, st)[rows["step"][0]] if rows else None)   # (the warm-up step is the call's first)
        torch.cuda.current_stream().wait_stream(warm)
        torch.cuda.synchronize()
        self._release_streamed()                             # (the warm-up fill of a host-resident cache has completed)
        st["latents"].copy_(saved)
        self._graphs[key] = G
        return G

    def _state_rows(self, G, st):
        """A call's plans -> the persistent plans of a row graph state, one per shape (R, a): made on first use as clones of the call's,
        otherwise the call's context, key counts and plan tables are copied into them -- and always the table active person -> set slot,
        which a call does not have.  -> the state's plans in the order of the call's."""
        slot, out = self._slot_table(st), []
        for p in st["rows"]["plans"]:
            key = (p["R"], p["a"])
            mine = G["rows"].get(key)
            if mine is None:
                clone = lambda t: t.clone() if t is not None else None
                mine = G["rows"][key] = dict(p, row_person_t=p["row_person_t"].clone(), table=p["table"].clone(), gnk=clone(p["gnk"]), gix=torch.empty_like(p["gix"]),
                                             ctx={**p["ctx"], "kv": {n: {kind: t.clone() for kind, t in ent.items()} for n, ent in p["ctx"]["kv"].items()}})
            else:
                for name in ("row_person_t", "table", "gnk"):
                    if mine[name] is not None:
                        mine[name].copy_(p[name])
                for n, ent in p["ctx"]["kv"].items():
                    for kind, t in ent.items():
                        mine["ctx"]["kv"][n][kind].copy_(t)
            mine["gix"].copy_(slot[p["persons_t"]])
            out.append(mine)
        return out

    def _state_step(self, G, par, j, plan=None):
        """One TryonNet step of a graph state on its persistent buffers, timestep slice j of set par (a row state's at its plan's shape:
        prefix views of tt and x_in): the warm-up, and what a capture records."""
        self._tryon_main(G, G["tt"] if plan is None else G["tt"][:plan["R"]], G["cf"], G["nz"], G["sets"][par]["step"][j], plan)

    def _graph(self, G, kind, par, j=0, plan=None):
        gk = (kind, par, j) + ((plan["R"], plan["a"]) if plan is not None else ())
        if gk in G["graphs"]:
            return G["graphs"][gk]
        keep = G["latents"].clone()
        torch.cuda.synchronize()                                     # nothing of this engine in flight while a capture starts
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=G["pools"][kind], capture_error_mode="thread_local"):
            if kind == "garm":                                   # j = timesteps in the batch
                self._garment_side(G, G["tgk"], G["sets"][par], j)
                self.stats["garment_batches"] -= 1               # captured, not run: replays are counted
            else:
                self._state_step(G, par, j, plan)
        G["latents"].copy_(keep)                                     # capture does not execute, but keep the state explicit
        G["graphs"][gk] = g
        return g

    def _graph_form(self, st, live, overlap):
        G = self._graph_state(st, live)
        if G["latents"] is not st["latents"]:
            _copy_state(G, dict(st, gix=self._slot_table(st)))                             # new call -> persistent buffers
        blocks, graphs = st["blocks"], G["graphs"]
        rows = st.get("rows")
        # capture everything this call needs before the loop (a capture must not interleave with work in flight on the side stream)
        if rows:                                             # ('tryon', p, j, R, a): the steps of this call, each at its plan's shape
            plans = self._state_rows(G, st)
            for bi, (s0, c) in enumerate(blocks):
                for j in range(c):
                    self._graph(G, "tryon", (bi & 1) if overlap and len(blocks) > 1 else 0, j, plans[rows["step"][s0 + j]])
        for p in ((0, 1) if overlap and len(blocks) > 1 else (0,)) if not rows else ():
            for j in range(st["k"]):
                self._graph(G, "tryon", p, j)
        if live:
            for bi, (_, c) in enumerate(blocks):                 # one GarmentNet graph per (set, batch size)
                self._graph(G, "garm", (bi & 1) if overlap else 0, c)

            def garment(bi, p):
                G["tgk"].copy_(st["temb_gk"][bi])
                self.stats["garment_batches"] += 1
                graphs[("garm", p, blocks[bi][1])].replay()
        else:                                                # in the GarmentNet graph's place in the stream / event order: the block out of the cache
            garment = self._cached_fill(st, G["sets"])
        tt, cf, nz = G["tt"], G["cf"], G["nz"]

        def step(i, j, p):
            plan = plans[rows["step"][i]] if rows else None
            if plan is None:
                tt.copy_(st["temb_t"][i])
            else:
                tt[:plan["R"]].copy_(rows["temb"][i])
            cf.copy_(st["coef"][i])
            if nz is not None:
                nz.copy_(st["steps_noise"][i])
            self._count_step(G, plan)
            graphs[("tryon", p, j) + ((plan["R"], plan["a"]) if plan is not None else ())].replay()

        return garment, step, G["latents"], (G["side"], G["ready"], G["free"]) if overlap else None

    @torch.no_grad()
    def denoise(self, st, use_graph=False, trace=None, overlap=False, on_step=None, host_transport="kernel"):
        """The loop.  Four execution forms with bit-identical results: {serial, two-stream overlap} x {eager, hipGraph replay}, each on a live
        GarmentNet or on a GarmentCache.  on_step(i, t, latents) runs after step i on the live latents (it may rewrite them in place); a true
        return value ends the loop (the reference's per-step callbacks and `interrupt`, tryon_pipeline.py:1766-1767,1840-1863: host code
        between two steps, which only the un-captured serial form can run, so it selects that form).  trace["step_latents"] receives a copy
        of the latents after every step.  Graph forms return their persistent latents buffer, eager forms st["latents"].
        host_transport: how a HOST-RESIDENT cache crosses the host link -- "kernel" (a kernel reads page-locked
        memory) or "copy" (the copy engines into a staging arena, one idmvton_kv_place launch per block); the same bits in the
        sets, the same graph states.  Any other value is a ValueError before anything is launched; on a device-resident cache or a live call
        the keyword has no effect.  A service sets it once."""
        self._check_host_transport(host_transport)
        if on_step is not None:
            use_graph = overlap = False
        st = dict(st, host_transport=host_transport)         # (read by _cached_fill alone: the same tensors, no key of a state or a set)
        live = st["gcache"] is None                          # the one place a call chooses where its garment K / V^T come from
        garment, step, latents, sync = (self._graph_form if use_graph else self._eager_form)(st, live, overlap)
        blocks = st["blocks"]

        def tryon(bi, p):
            s0, c = blocks[bi]
            for j in range(c):
                i = s0 + j
                step(i, j, p)
                if trace is not None:
                    trace.setdefault("step_latents", []).append(latents.clone())
                if on_step is not None and on_step(i, int(st["timesteps"][i]), latents):
                    return True

        if sync is None:
            drive_blocks(blocks, garment, tryon)
        else:
            drive_blocks(blocks, garment, tryon, torch.cuda.current_stream(), *sync)
        return latents

    @torch.no_grad()
    def decode(self, latents):
        self._release_streamed()
        img = self.vae.decode(latents / self.vae.cfg.scaling_factor)                       # :1876
        return (img / 2 + 0.5).clamp(0, 1)                                                 # postprocess

    @torch.no_grad()
    def __call__(self, *, return_latents=False, use_graph=False, overlap=False, timing=None, on_step=None, host_transport="kernel", **kw):
        """timing: a list that receives one (start, prepared, denoised, decoded) tuple of HIP events recorded on the current stream
        (bench.py: the loop's share of a timed call without a second, instrumented run).  host_transport: see denoise."""
        self._check_host_transport(host_transport)           # before prepare launches anything
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timing is not None else None
        if ev:
            ev[0].record()
        st = self.prepare(**kw)
        if ev:
            ev[1].record()
        lat = self.denoise(st, use_graph=use_graph, overlap=overlap, on_step=on_step, host_transport=host_transport)
        if ev:
            ev[2].record()
        out = lat if return_latents else self.decode(lat)
        if ev:
            ev[3].record()
            timing.append(tuple(ev))
        return out
