"""TryonNet / GarmentNet executed on the HIP kernels (NHWC, token-major, no layout transposes anywhere).

Host-side mirror of /root/reference/src/unet_hacked_tryon.py:1006-1395 and src/unet_hacked_garmnet.py:917-1284: same
topology walk, same state-dict keys, every arithmetic op a C-ABI call (ops.py).  Exact savings taken:

  * self-attention computes only the N kept query rows (reference discards rows N..2N, attentionhacked_tryon.py:348);
  * the CFG-unconditional half's all-zero garment features (tryon_pipeline.py:1796) are never materialised: the
    attention kernel adds their closed-form contribution (N keys, logit 0, value 0);
  * skip-connection torch.cat's (unet_block_hacked_tryon.py:2346,2482) are dual-pointer reads;
  * text / image-token K and V of every attn2 and add_embedding are step-invariant: projected once per call;
  * GarmentNet stops after its last exported norm1 (everything after it is dead: unet_hacked_garmnet.py:1267-1284).
"""
import math
import os

import torch

from . import ffi, ops
from .config import UNetConfig, unet_topology
from .weights import conv_weight_nhwc, conv_weight_nhwc_padded, interleave_geglu


def _pad64(c):
    return (c + 63) // 64 * 64


class _Conv:
    """Prepared conv: GEMM weight [Cout][taps*Cin_pad (+ shortcut Cin)] and bias (fp16/bf16)."""

    def __init__(self, sd, name, cin_pad=None, shortcut=None, pad_out_to=None):
        w = sd[name + ".weight"]
        b = sd[name + ".bias"]
        self.k = w.shape[-1]
        self.cin = w.shape[1]
        self.cin_pad = cin_pad or self.cin
        wk = conv_weight_nhwc_padded(w, self.cin_pad) if self.cin_pad != self.cin else conv_weight_nhwc(w)
        if shortcut is not None:                      # fused 1x1 conv_shortcut: extra K columns, biases add
            ws = sd[shortcut + ".weight"]
            wk = torch.cat([wk, ws.reshape(ws.shape[0], ws.shape[1])], dim=1)
            b = (b.float() + sd[shortcut + ".bias"].float()).to(b.dtype)
        self.cout = w.shape[0]
        if pad_out_to and pad_out_to > self.cout:     # N must be a multiple of 4
            wk = torch.cat([wk, torch.zeros(pad_out_to - self.cout, wk.shape[1], dtype=wk.dtype, device=wk.device)])
            b = torch.cat([b, torch.zeros(pad_out_to - self.cout, dtype=b.dtype, device=b.device)])
        self.w = wk.contiguous()
        self.b = b.contiguous()
        self.n = self.w.shape[0]


class HipUNet:
    def __init__(self, cfg: UNetConfig, state_dict, dtype=torch.bfloat16, device="cuda", stream_f32=False, attn_fp8=False, fuse_xattn=True):
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        # stream_f32: inside a Transformer2DModel the block-to-block hidden state (three `+ hidden_states` per block,
        # attentionhacked_tryon.py:348,384,412) stays fp32 from proj_in to the last block's ff.net.2, whose output is rounded once
        # for proj_out (its GEMM operand).  Off by default: the reference's fp16 autocast rounds the stream after every add, and
        # measured at full size the option lowers the latent error by 10-35 % for 2.4 % of throughput --
        # operand rounding inside the branches, not the stream, is what bf16 storage costs.
        self.stream_f32 = bool(stream_f32)
        # (LayerNorm folded into the neighbouring GEMMs -- row statistics emitted by the producer's epilogue, gamma folded into the consumer's
        #  weights -- was built and measured in rounds 3 and 4 in two forms, +-0 .. -3 % end to end, and removed in
        #  round 5: norm1 / norm2 / norm3 run as LayerNorm kernels.)
        # attn_fp8 (BASELINE.json configs[4]: "fp16 + fp8 MFMA attention"): every self-attention (attn1) runs on e4m3 operands through
        # the block-scaled MFMA (csrc/attention_f8.hip); q, k, v are quantised with power-of-two scales 2^eq, 2^ek, 2^ev right after the
        # QKV projection.  Cross-attention (93 keys) and everything else stay 16-bit.  6e-2 .. 1e-1 max-rel per attention output (e4m3: 3 mantissa bits).
        self.attn_fp8 = bool(attn_fp8)
        # fuse_xattn: attn2.to_q -> cross-attention (77 text [+ 16 image] keys) as ONE launch, the attention being the projection's epilogue
        # (csrc/xattn.cuh).  Same arithmetic as the two launches (q rounded once to the storage type, fp32 logits and softmax, P rounded for P.V)
        self.fuse_xattn = bool(fuse_xattn) and os.environ.get("IDMVTON_FUSE_XATTN", "1") != "0"
        self.f8_exp = (2, 2, 2)
        self.f8_fused = os.environ.get("IDMVTON_F8_FUSED", "1") != "0"     # 0: project in 16 bits, then idmvton_quant_f8 (the round-3 form; A/B only)
        self.topo = unet_topology(cfg)
        sd = {k: v.to(device=self.device, dtype=dtype) for k, v in state_dict.items() if not k.startswith("encoder_hid_proj.")}
        self.sd = sd
        for h, c in zip(cfg.num_attention_heads, cfg.block_out_channels):
            assert c % 64 == 0 and (c // h == 64), "HIP attention kernels are specialised for head_dim 64"
        self.tryon = cfg.mode == "tryon"
        self.ip_scale = 1.0                              # IPAttnProcessor2_0.scale (ip_adapter/attention_processor.py:1995): hidden = text + scale * ip
        self.cin_pad = _pad64(cfg.in_channels)
        self._prep()
        self._gn_stats = torch.empty(ops.GN_STATS_DOUBLES, dtype=torch.float64, device=self.device)
        self._ctx = None

    # ------------------------------------------------------------------------------------------------ weight prep
    def _prep(self):
        sd, cfg = self.sd, self.cfg
        self.conv_in = _Conv(sd, "conv_in", cin_pad=self.cin_pad)
        self.res = {}
        self.tf = {}
        temb_w, temb_b, self.temb_slices, off = [], [], {}, 0

        def prep_res(p, cin, cout):
            sc = p + ".conv_shortcut" if cin != cout else None
            self.res[p] = dict(conv1=_Conv(sd, p + ".conv1"), conv2=_Conv(sd, p + ".conv2", shortcut=sc), cin=cin, cout=cout)
            nonlocal off
            temb_w.append(sd[p + ".time_emb_proj.weight"])
            temb_b.append(sd[p + ".time_emb_proj.bias"])
            self.temb_slices[p] = (off, cout)
            off += cout

        def prep_tf(p, ch, n_tf, heads, level):
            """level = index of the resolution the transformer runs at (0 = the latent size, +1 per Downsample2D): recorded from the
            topology walk, not inferred from the channel count (block_out_channels may repeat a width)."""
            blocks = []
            for k in range(n_tf):
                b = f"{p}.transformer_blocks.{k}"
                d = dict(heads=heads)
                d["qkv"] = torch.cat([sd[f"{b}.attn1.to_q.weight"], sd[f"{b}.attn1.to_k.weight"], sd[f"{b}.attn1.to_v.weight"]]).contiguous()
                d["kv_text"] = torch.cat([sd[f"{b}.attn2.to_k.weight"], sd[f"{b}.attn2.to_v.weight"]]).contiguous()
                if self.tryon:
                    d["kv_ip"] = torch.cat([sd[f"{b}.attn2.processor.to_k_ip.weight"], sd[f"{b}.attn2.processor.to_v_ip.weight"]]).contiguous()
                d["ff1_w"], d["ff1_b"] = interleave_geglu(sd[f"{b}.ff.net.0.proj.weight"], sd[f"{b}.ff.net.0.proj.bias"])
                d["p"] = b
                blocks.append(d)
            self.tf[p] = dict(blocks=blocks, ch=ch, heads=heads, level=level)

        level = 0
        for i, blk in enumerate(self.topo["down"]):
            for j, (ci, co) in enumerate(blk["resnets"]):
                prep_res(f"down_blocks.{i}.resnets.{j}", ci, co)
                if blk["attn"]:
                    prep_tf(f"down_blocks.{i}.attentions.{j}", blk["ch"], blk["n_tf"], blk["heads"], level)
            if blk["down"]:
                self.res[f"down_blocks.{i}.downsamplers.0.conv"] = _Conv(sd, f"down_blocks.{i}.downsamplers.0.conv")
                level += 1
        m = self.topo["mid"]
        prep_res("mid_block.resnets.0", m["ch"], m["ch"])
        prep_tf("mid_block.attentions.0", m["ch"], m["n_tf"], m["heads"], level)
        prep_res("mid_block.resnets.1", m["ch"], m["ch"])
        for i, blk in enumerate(self.topo["up"]):
            if self.tryon or blk["attn"]:              # GarmentNet never executes non-attention up blocks
                for j, (rin, skip, co) in enumerate(blk["resnets"]):
                    prep_res(f"up_blocks.{i}.resnets.{j}", rin + skip, co)
                    if blk["attn"]:
                        prep_tf(f"up_blocks.{i}.attentions.{j}", blk["ch"], blk["n_tf"], blk["heads"], level)
                if blk["up"]:
                    self.res[f"up_blocks.{i}.upsamplers.0.conv"] = _Conv(sd, f"up_blocks.{i}.upsamplers.0.conv")
            if blk["up"]:
                level -= 1
        # transformer blocks in traversal order == GarmentNet feature order (unet_hacked_tryon.py:1254 running index)
        self.block_order = [blk for tf in self.tf.values() for blk in tf["blocks"]]
        self.temb_w = torch.cat(temb_w).contiguous()          # one GEMM for every resnet's time_emb_proj
        self.temb_b = torch.cat(temb_b).contiguous()
        if self.tryon:
            self.conv_out = _Conv(sd, "conv_out", pad_out_to=_pad64(cfg.out_channels) if cfg.out_channels % 4 else None)

    # ------------------------------------------------------------------------------------------------ per-call setup
    def time_embeddings(self, timesteps, batch, added_cond=None):
        """emb[step] = time_embedding(Timesteps(t)) (+ add_embedding(...)), then EVERY resnet's time_emb_proj(silu(emb))
        in one GEMM per step (unet_hacked_tryon.py:1118-1213; diffusers ResnetBlock2D).  Returns [steps][batch][sum Cout].
        Runs once per pipeline call, outside the denoising loop (the timestep schedule is known up front)."""
        cfg, sd, dt = self.cfg, self.sd, self.dtype
        ts = torch.as_tensor(timesteps, dtype=torch.float32, device=self.device).reshape(-1)
        half = cfg.block_out_channels[0] // 2
        freq = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=self.device) / half)
        ang = ts[:, None] * freq[None, :]
        t_emb = torch.cat([torch.cos(ang), torch.sin(ang)], dim=-1).to(dt)            # flip_sin_to_cos
        S = ts.numel()
        mp = max(S, 1)
        e = ops.linear(t_emb.contiguous(), sd["time_embedding.linear_1.weight"], bias=sd["time_embedding.linear_1.bias"])
        e = ops.linear(torch.nn.functional.silu(e.float()).to(dt), sd["time_embedding.linear_2.weight"], bias=sd["time_embedding.linear_2.bias"])
        emb = e[:, None, :].expand(S, batch, -1)                                        # timesteps.expand(batch)
        if cfg.addition_embed_type == "text_time":
            text_embeds, time_ids = added_cond["text_embeds"], added_cond["time_ids"]
            h2 = cfg.addition_time_embed_dim // 2
            f2 = torch.exp(-math.log(10000.0) * torch.arange(h2, dtype=torch.float32, device=self.device) / h2)
            a2 = time_ids.to(self.device).float().flatten()[:, None] * f2[None, :]
            te = torch.cat([torch.cos(a2), torch.sin(a2)], dim=-1).reshape(batch, -1)
            add = torch.cat([text_embeds.to(self.device).float(), te], dim=-1).to(dt).contiguous()
            a = ops.linear(add, sd["add_embedding.linear_1.weight"], bias=sd["add_embedding.linear_1.bias"])
            a = ops.linear(torch.nn.functional.silu(a.float()).to(dt), sd["add_embedding.linear_2.weight"], bias=sd["add_embedding.linear_2.bias"])
            emb = (emb.float() + a.float()[None]).to(dt)
        x = torch.nn.functional.silu(emb.float()).to(dt).reshape(S * batch, -1).contiguous()
        out = ops.linear(x, self.temb_w, bias=self.temb_b)
        return out.reshape(S, batch, -1)

    def encode_context(self, text, ip=None):
        """Step-invariant cross-attention K / V^T for every attn2 (ip_adapter/attention_processor.py:1957-1958,1978-1979).
        text: [B][77][xd]; ip: [B][16][xd] image tokens (TryonNet).  Rows are padded to a multiple of 16 with zeros."""
        dt, dev = self.dtype, self.device
        B, nt, xd = text.shape
        rt = (nt + 31) // 32 * 32                            # key-order V^T needs multiples of 16; the fused cross-attention reads K in 32-row blocks
        tpad = torch.zeros(B, rt, xd, dtype=dt, device=dev)
        tpad[:, :nt] = text.to(dev, dt)
        ctx = dict(B=B, nt=nt, rt=rt, kv={})
        if ip is not None:
            ni = ip.shape[1]
            ri = (ni + 31) // 32 * 32
            ipad = torch.zeros(B, ri, xd, dtype=dt, device=dev)
            ipad[:, :ni] = ip.to(dev, dt)
            ctx.update(ni=ni, ri=ri)
        for p, tf in self.tf.items():
            C = tf["ch"]
            for blk in tf["blocks"]:
                kt = torch.empty(B * rt, C, dtype=dt, device=dev)
                vtt = torch.empty(B, C, rt, dtype=dt, device=dev)
                ops.linear(tpad.reshape(B * rt, xd), blk["kv_text"], out=kt, vt=vtt, vt_n0=C, vt_tokens=rt)
                ent = dict(kt=kt, vtt=vtt)
                if ip is not None:
                    ki = torch.empty(B * ri, C, dtype=dt, device=dev)
                    vti = torch.empty(B, C, ri, dtype=dt, device=dev)
                    ops.linear(ipad.reshape(B * ri, xd), blk["kv_ip"], out=ki, vt=vti, vt_n0=C, vt_tokens=ri)
                    ent.update(ki=ki, vti=vti)
                ctx["kv"][blk["p"]] = ent
        return ctx

    # ------------------------------------------------------------------------------------------------ building blocks
    def _gn(self, xa, xb, name, eps, silu):
        sd = self.sd
        return ops.groupnorm(xa, sd[name + ".weight"], sd[name + ".bias"], self.cfg.norm_num_groups, eps, silu,
                             self._gn_stats, x2=xb)

    def _conv3(self, x, cv, B, H, W, stride=1, ups=False, extra_segs=(), out_hw=None, **kw):
        """out_hw (ups only): the skip tensor's H x W when it is odd -- diffusers' `upsample_size` (unet_hacked_tryon.py:1357-1379): the fused
        nearest upsample then produces 2H - 1 rows / 2W - 1 columns instead of 2H / 2W."""
        Ho, Wo = (out_hw or (H * 2, W * 2)) if ups else ((H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1)
        segs = ops.conv_segs(x, 3, 1, length=cv.cin_pad) + list(extra_segs)
        out = ops.gemm_conv(segs, cv.w, B * Ho * Wo, Ho=Ho, Wo=Wo, Hi=H, Wi=W, stride=stride, ups=ups, bias=cv.b, **kw)
        return out.view(B, Ho * Wo, cv.n), Ho, Wo

    def _resnet(self, p, xa, xb, temb, B, H, W):
        """diffusers ResnetBlock2D.  xa (+xb): input, virtually concatenated along channels."""
        r = self.res[p]
        eps = self.cfg.norm_eps
        g1 = self._gn(xa, xb, p + ".norm1", eps, True)
        off, co = self.temb_slices[p]
        h, _, _ = self._conv3(g1, r["conv1"], B, H, W, rowbias=temb[:, off:off + co], rowbias_ld=temb.stride(0),
                              rows_per_group=H * W)
        g2 = self._gn(h, None, p + ".norm2", eps, True)
        if r["cin"] != r["cout"]:                    # 1x1 conv_shortcut fused as extra centre-tap K segments
            extra = [ops.SegSpec(xa, 0, xa.shape[-1])] + ([ops.SegSpec(xb, 0, xb.shape[-1])] if xb is not None else [])
            out, _, _ = self._conv3(g2, r["conv2"], B, H, W, extra_segs=extra)
        else:
            out, _, _ = self._conv3(g2, r["conv2"], B, H, W, res=xa.reshape(B * H * W, -1))
        return out

    def _block(self, blk, hs, B, N, C, ctx, garment, feats_out, stop=None, last=False, nk=None):
        """BasicTransformerBlock: tryon src/attentionhacked_tryon.py:284-415, garmnet src/attentionhacked_garmnet.py:284-406.
        N = token ROWS per image (a multiple of 16: the V^T layout works in groups of 16 keys); nk = the real token count when the rows
        are padded (sizes whose H*W is not a multiple of 16: rows nk..N-1 hold finite filler that no key / output ever reads)."""
        sd, p, heads = self.sd, blk["p"], blk["heads"]
        dt, dev = self.dtype, self.device
        M = B * N
        nk = N if nk is None else nk
        feat = None
        if not self.tryon:                                       # exported norm1 output (garmnet :321-322)
            fb = garment.get("feats_buf") if garment else None
            feat = fb[len(feats_out)][:B].view(M, C) if fb is not None else torch.empty(M, C, dtype=dt, device=dev)
        # attn_fp8: the projections write the e4m3 operands themselves (IDMVTON_IO_OUT_F8: one rounding, no quant launches) when the token
        # rows are whole 64-key tiles; other sizes project in 16 bits and quantise with idmvton_quant_f8
        f8 = self._f8_fused(N)
        eq, ek, ev = self.f8_exp
        f8kw = dict(f8=(2.0 ** ek, 2.0 ** ev)) if f8 else {}
        qk = torch.empty(M, 2 * C, dtype=torch.uint8 if f8 else dt, device=dev)
        vt = torch.empty(B, C, N, dtype=torch.uint8 if f8 else dt, device=dev)
        qcs = ops.QSCALE * (2.0 ** (eq - ek) if f8 else 1.0)     # q columns: softmax scale (and 2^eq over the 2^ek every `out` column gets)
        # q columns leave the GEMM multiplied by softmax_scale * log2(e) (fp32, before the one rounding to the storage dtype)
        n1 = ops.layernorm(hs, sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5, out2=feat)
        if feat is not None:
            feats_out.append(feat.view(B, N, C))
            if stop is not None and len(feats_out) >= stop:
                return None                              # GarmentNet: everything after the last export is dead compute
        ops.linear(n1, blk["qkv"], out=qk, vt=vt, vt_n0=2 * C, vt_tokens=N, colscale_n=C, colscale=qcs, **f8kw)
        segs = [dict(k=qk[:, C:], vt=vt, nk=nk, ldk=2 * C, ldvt=N, k_rows=N)]
        if self.tryon:
            # the garment segment has its own geometry (attentionhacked_tryon.py:334 joins the two along the token axis only): gnk real tokens
            # in Ng = round16(gnk) rows per garment, whatever the person's N
            gnk = garment["nk"][garment["idx"]] if garment.get("nk") is not None else None
            if garment.get("kv") is not None:                   # K / V^T of the garment tokens projected ahead of time
                kg, vtg = garment["kv"][garment["idx"]]         # (project_garment_kv, on the GarmentNet stream)
                Bg, Ng = vtg.shape[0], vtg.shape[2]
                if gnk is None:
                    if Ng != N:
                        raise ValueError(f"garment K / V^T of {Ng} token rows against {N} own rows: pass garment_hw (the garment's latent size)")
                    gnk = nk
            else:
                g = garment["feats"][garment["idx"]]            # [Bg][Ng][C] of any Ng (or [Bg][gnk][C]: reference-shaped features of a padded size)
                Bg = g.shape[0]
                if gnk is None:                                  # engine-shaped rows of the person's size, else the rows are the real tokens
                    gnk = nk if g.shape[1] == N else g.shape[1]
                Ng = ops.round16(gnk)
                if g.shape[1] != Ng:
                    gp = torch.zeros(Bg, Ng, C, dtype=dt, device=dev)
                    gp[:, :g.shape[1]] = g
                    g = gp
                f8g = self._f8_fused(Ng)
                kg = torch.empty(Bg * Ng, C, dtype=torch.uint8 if f8g else dt, device=dev)
                vtg = torch.empty(Bg, C, Ng, dtype=torch.uint8 if f8g else dt, device=dev)
                ops.linear(g.reshape(Bg * Ng, C), blk["qkv"][C:], out=kg, vt=vtg, vt_n0=C, vt_tokens=Ng,
                           **(dict(f8=(2.0 ** ek, 2.0 ** ev)) if f8g else {}))
            garment["idx"] += 1
            gix = garment.get("index")
            P = gix.numel() if gix is not None else garment.get("persons") or Bg   # conditional batches (GarmentCache calls: P persons, Bg = G garments)
            gseg = dict(k=kg, vt=vtg, nk=gnk, ldk=C, ldvt=Ng, k_rows=Ng, b0=B - P)
            if gix is not None:                                  # a pooled segment: conditional row i reads garment index[i] of the Bg, whatever Bg is to P
                gseg.update(nb=Bg, index=gix)
            elif Bg < P:                                         # a shared segment: conditional row i reads garment i % G
                gseg["nb"] = Bg
            if garment.get("nk_table") is not None:              # a ragged segment: batch b has nk_table[b] of the slot's gnk keys
                gseg["nk_table"] = garment["nk_table"][garment["idx"] - 1]
            segs.append(gseg)
        att = torch.empty(M, C, dtype=dt, device=dev)
        if self.attn_fp8:
            segs8 = []
            for sg in segs:                                      # each segment with its own token rows: e4m3 from its projection, or quantised here
                Bs, Ns = sg["vt"].shape[0], sg["k_rows"]
                if sg["k"].dtype == torch.uint8:                                            # written as e4m3 by its projection
                    segs8.append(dict(k8=sg["k"], vt8=sg["vt"], nk=sg["nk"], ldk=sg["ldk"], ldvt=sg["ldvt"], k_rows=Ns, b0=sg.get("b0", 0), nb=sg.get("nb", 0),
                                      index=sg.get("index"), nk_table=sg.get("nk_table")))
                    continue
                k8 = ops.quant_f8(sg["k"], 2.0 ** ek)                                   # [Bs*Ns][C] (row stride ldk)
                vt8 = ops.quant_f8(sg["vt"].reshape(Bs * C, Ns), 2.0 ** ev, mode=1)     # 16-bit key order -> fp8 slot order (a ragged slot: whole)
                segs8.append(dict(k8=k8, vt8=vt8, nk=sg["nk"], ldk=C, ldvt=vt8.shape[1], k_rows=Ns, b0=sg.get("b0", 0), nb=sg.get("nb", 0), index=sg.get("index"),
                                  nk_table=sg.get("nk_table")))
            if f8:
                q8, ldq8 = qk, 2 * C
            else:
                q8, ldq8 = ops.quant_f8(qk[:, :C], 2.0 ** eq), C
            ops.attention_f8(q8, att, segs8, heads, qk_scale_exp=-(eq + ek), v_scale_exp=-ev, B=B, Nq=N, ldq=ldq8, ldo=C)
        else:
            ops.attention(qk, att, segs, heads, B=B, Nq=N, ldq=2 * C, ldo=C, q_prescaled=True)
        f32 = hs.dtype == torch.float32                          # the fp32 residual stream (see __init__)
        hs = ops.linear(att, sd[p + ".attn1.to_out.0.weight"], bias=sd[p + ".attn1.to_out.0.bias"], res=hs, out_f32=f32)
        # cross attention
        kv = ctx["kv"][p]
        seg_t = dict(k=kv["kt"], vt=kv["vtt"], nk=ctx["nt"], ldk=C, ldvt=ctx["rt"], k_rows=ctx["rt"])
        xsegs = [seg_t] + ([dict(k=kv["ki"], vt=kv["vti"], nk=ctx["ni"], ldk=C, ldvt=ctx["ri"], k_rows=ctx["ri"])] if self.tryon else [])
        # (not for the timestep-batched GarmentNet at the 1280-channel level: at M = 9216 the plain projection runs on the 256x256 tile at twice
        #  the rate of the 128-column tiles the fused form needs -- 55 us for the two launches against 60 fused, profiles/r04_xattn_probe_*.log)
        if self.fuse_xattn and N % 32 == 0 and not (C >= 1280 and M >= 8192) and \
                all(sg["nk"] <= (96, 32)[i] and sg["k_rows"] >= (sg["nk"] + 31) // 32 * 32 for i, sg in enumerate(xsegs)):
            # (96 text keys / 32 image-prompt keys are what the fused epilogue holds; a larger segment takes the two-launch path below)
            # attn2.to_q with the cross-attention as its epilogue (csrc/xattn.cuh): q never leaves the registers, no attention launch
            if "q2_xw" not in blk:
                blk["q2_xw"] = ops.xattn_q_weight(sd[p + ".attn2.to_q.weight"])
            n2 = ops.layernorm(hs, sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], 1e-5)
            att2 = ops.linear(n2, blk["q2_xw"], xattn=dict(segs=xsegs, tokens=N, ip_scale=self.ip_scale))
        else:
            n2 = ops.layernorm(hs, sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], 1e-5)
            q2 = ops.linear(n2, sd[p + ".attn2.to_q.weight"])
            att2 = torch.empty(M, C, dtype=dt, device=dev)
            if self.tryon:
                ops.attention(q2, att2, xsegs, heads, mode=ffi.ATTN_CROSS, ip_scale=self.ip_scale, B=B, Nq=N, ldq=C, ldo=C)
            else:
                ops.attention(q2, att2, xsegs, heads, B=B, Nq=N, ldq=C, ldo=C)
        hs = ops.linear(att2, sd[p + ".attn2.to_out.0.weight"], bias=sd[p + ".attn2.to_out.0.bias"], res=hs, out_f32=f32)
        # feed-forward (GEGLU fused into the first GEMM's epilogue)
        n3 = ops.layernorm(hs, sd[p + ".norm3.weight"], sd[p + ".norm3.bias"], 1e-5)
        gg = ops.linear(n3, blk["ff1_w"], bias=blk["ff1_b"], geglu=True)
        hs = ops.linear(gg, sd[p + ".ff.net.2.weight"], bias=sd[p + ".ff.net.2.bias"], res=hs, out_f32=f32 and not last)
        return hs

    def _transformer(self, p, x, B, H, W, ctx, garment, feats_out, stop_after_feats=None):
        """Transformer2DModel (src/transformerhacked_tryon.py:246-467), NHWC so no permutes."""
        sd, tf = self.sd, self.tf[p]
        C, N = tf["ch"], H * W
        Np = ops.round16(N)                                  # token rows per image inside the transformer (V^T works in groups of 16 keys)
        g = self._gn(x, None, p + ".norm", 1e-6, False)
        if Np == N:
            hs = ops.linear(g.reshape(B * N, C), sd[p + ".proj_in.weight"], bias=sd[p + ".proj_in.bias"], out_f32=self.stream_f32)
        else:
            # H*W not a multiple of 16 (e.g. 320x320 -> 10x10 tokens at the coarsest level): proj_in as a 1x1 convolution from an N-pixel row
            # to an Np-pixel row per image -- rows N..Np-1 read outside the image (zeros -> bias): finite filler the attention masks as keys
            hs = ops.gemm_conv([ops.SegSpec(g, 0, C)], sd[p + ".proj_in.weight"], B * Np, Ho=1, Wo=Np, Hi=1, Wi=N, bias=sd[p + ".proj_in.bias"],
                               out_f32=self.stream_f32)
        for blk in tf["blocks"]:
            hs = self._block(blk, hs, B, Np, C, ctx, garment, feats_out, stop_after_feats, last=blk is tf["blocks"][-1], nk=N)
            if hs is None:
                return None
        if Np == N:
            out = ops.linear(hs, sd[p + ".proj_out.weight"], bias=sd[p + ".proj_out.bias"], res=x.reshape(B * N, C))
        else:
            out = ops.gemm_conv([ops.SegSpec(hs.view(B, Np, C), 0, C)], sd[p + ".proj_out.weight"], B * N, Ho=1, Wo=N, Hi=1, Wi=Np,
                                bias=sd[p + ".proj_out.bias"], res=x.reshape(B * N, C))
        return out.view(B, N, C)

    def feature_tokens(self, h, w):
        """Real token count of each exported / consumed garment feature at latent size h x w (features are returned with round16 rows)."""
        lv = [(h, w)]
        for _ in range(len(self.cfg.block_out_channels) - 1):
            lv.append(((lv[-1][0] + 1) // 2, (lv[-1][1] + 1) // 2))
        return [lv[tf["level"]][0] * lv[tf["level"]][1] for tf in self.tf.values() for _ in tf["blocks"]]

    def num_features(self):
        return sum(len(t["blocks"]) for t in self.tf.values())

    def _f8_fused(self, N):
        return self.attn_fp8 and self.f8_fused and N % 64 == 0

    def project_garment_kv(self, feats, out=None):
        """TryonNet only: attn1.to_k / to_v of every block applied to the matching GarmentNet feature (the garment half of
        the concatenated self-attention input, attentionhacked_tryon.py:334-342) -> [(K [Bg*N][C], V^T [Bg][C][N])] * 70.
        It depends only on GarmentNet's output, so the engine runs it on the GarmentNet stream, one step ahead of TryonNet."""
        assert self.tryon and len(feats) == len(self.block_order)
        res = []
        for i, (blk, g) in enumerate(zip(self.block_order, feats)):
            Bg, N, C = g.shape
            f8 = self._f8_fused(N)                               # e4m3 straight from the projection (see _block)
            if out is not None:
                kg, vtg = out[i][0][:Bg * N], out[i][1][:Bg]     # the persistent set is sized for the largest block
            else:
                kg = torch.empty(Bg * N, C, dtype=torch.uint8 if f8 else self.dtype, device=self.device)
                vtg = torch.empty(Bg, C, N, dtype=torch.uint8 if f8 else self.dtype, device=self.device)
            f8kw = dict(f8=(2.0 ** self.f8_exp[1], 2.0 ** self.f8_exp[2])) if f8 else {}
            ops.linear(g.reshape(Bg * N, C), blk["qkv"][C:], out=kg, vt=vtg, vt_n0=C, vt_tokens=N, **f8kw)
            res.append((kg, vtg))
        return res

    def weights_id(self, select=None):
        """Identity of this weight set (or of the tensors whose state-dict key satisfies `select`) in its storage dtype: see
        garment_cache.weights_fingerprint.  Computed once per selection and kept."""
        from .garment_cache import weights_fingerprint
        ids = self.__dict__.setdefault("_weights_ids", {})
        key = getattr(select, "__name__", None) if select is not None else "all"
        if key not in ids:
            ids[key] = weights_fingerprint({k: v for k, v in self.sd.items() if select is None or select(k)})
        return ids[key]

    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, x, temb, ctx, B, H, W, garment_feats=None, garment_kv=None, feats_buf=None, garment_persons=None, garment_hw=None,
                garment_index=None, garment_nk=None):
        """x: NHWC [B][H*W][cin_pad] (channels >= in_channels zero); temb: [B][sum Cout] (time_embeddings()[step]);
        ctx: encode_context(); garment_feats: list of [Bg][Ng][C] (Bg <= B; batches < B-Bg see all-zero features).
        garment_hw = the garment's own latent (gh, gw) when it is not (H, W): its features have feature_tokens(gh, gw) real tokens per level
        in round16 rows.  None: the person's size -- or, for garment_feats whose rows are neither N nor round16(N), the rows themselves
        (reference-shaped features of a garment of another size).
        garment_persons = P (with garment_kv of G = Bg garments, P % G == 0): the last P batches are conditional and row i of them reads garment
        i % G through a shared attention segment (GarmentCache calls); None: P = Bg, one garment entry per conditional batch.
        garment_index = an int32 device tensor of P entries (with garment_kv or garment_feats of any Bg >= 1 garments): the last P batches are
        conditional and row i of them reads garment garment_index[i] through an indexed attention segment -- no relation between Bg and P, and
        the table is read by the kernels, so a captured forward follows its contents.
        garment_nk = an int32 device tensor [features][B] (contiguous): row f holds, per batch, the real token count of garment feature f for
        that batch -- garments of several sizes in slots of garment_hw's size (the rows of garment_kv / garment_feats), each at the front of
        its slot.  Both CFG halves carry their person's count: an unconditional row counts the zero features of its own garment's shape.
        Returns (noise NHWC [B][H*W][n_out] for TryonNet | None, exported features for GarmentNet)."""
        topo = self.topo
        garment = dict(feats=garment_feats, kv=garment_kv, feats_buf=feats_buf, idx=0, persons=garment_persons, index=garment_index, nk_table=garment_nk,
                       nk=self.feature_tokens(*garment_hw) if garment_hw is not None and self.tryon else None)
        feats = []
        stop = None if self.tryon else self.num_features()
        h, _, _ = self._conv3(x, self.conv_in, B, H, W)
        skips = [(h, H, W)]
        for i, blk in enumerate(topo["down"]):
            for j in range(len(blk["resnets"])):
                h = self._resnet(f"down_blocks.{i}.resnets.{j}", h, None, temb, B, H, W)
                if blk["attn"]:
                    h = self._transformer(f"down_blocks.{i}.attentions.{j}", h, B, H, W, ctx, garment, feats)
                skips.append((h, H, W))
            if blk["down"]:
                h, H, W = self._conv3(h, self.res[f"down_blocks.{i}.downsamplers.0.conv"], B, H, W, stride=2)
                skips.append((h, H, W))
        h = self._resnet("mid_block.resnets.0", h, None, temb, B, H, W)
        h = self._transformer("mid_block.attentions.0", h, B, H, W, ctx, garment, feats)
        h = self._resnet("mid_block.resnets.1", h, None, temb, B, H, W)
        for i, blk in enumerate(topo["up"]):
            if not self.tryon and not blk["attn"]:
                continue
            for j in range(len(blk["resnets"])):
                s, sh, sw = skips.pop()
                assert (sh, sw) == (H, W), "skip / upsample size mismatch"
                h = self._resnet(f"up_blocks.{i}.resnets.{j}", h, s, temb, B, H, W)
                if blk["attn"]:
                    h = self._transformer(f"up_blocks.{i}.attentions.{j}", h, B, H, W, ctx, garment, feats, stop)
                    if h is None:
                        return None, feats
            if blk["up"]:
                # `upsample_size` (unet_hacked_tryon.py:1084-1090,1357-1379): the next skip's H x W, which is 2H - 1 / 2W - 1 for an odd level
                tgt = (skips[-1][1], skips[-1][2]) if skips else (2 * H, 2 * W)
                h, H, W = self._conv3(h, self.res[f"up_blocks.{i}.upsamplers.0.conv"], B, H, W, ups=True, out_hw=tgt)
        if not self.tryon:
            return None, feats
        g = self._gn(h, None, "conv_norm_out", self.cfg.norm_eps, True)
        out, _, _ = self._conv3(g, self.conv_out, B, H, W)
        return out, feats
