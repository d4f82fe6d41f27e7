"""CLIP text tower on the HIP operators, with trainable LoRA on its attention projections (--train_text_encoder_lora) or trained in
full (--tune_text_encoder: `ClipTextBank`).

Mirrors transformers' `CLIPTextModel` forward as the reference calls it (`TrainableSDPipeline.py:325-326`:
`text_encoder(ids, attention_mask=None)[0]`): token + position embedding, pre-LN blocks (layer_norm1 -> q / k / v with bias ->
causal self-attention -> out_proj -> residual; layer_norm2 -> fc1 -> quick-GELU -> fc2 -> residual) and the final layer norm.
The causal mask is the only mask: the reference passes no key-padding mask.  The frozen weights carry no gradient, the ids carry
none; the LoRA factors of a `ClipLoRABank` do (`LoraLoaderMixin._modify_text_encoder`, training_utils/pipeline.py:117-119,176-184:
fp32 LoRA on q_proj / k_proj / v_proj / out_proj of every layer at scale 1, the MLP left alone - `patch_mlp` defaults to False).
Tokenisation stays outside: the encoder takes input ids.
"""
from __future__ import annotations

import torch

from . import ops, refresh
from .config import ClipTextConfig

PROJS = ("q_proj", "k_proj", "v_proj", "out_proj")

# The ONE table of LoRA key names.  These are diffusers' `text_encoder_lora_state_dict` names as of diffusers 0.22, written from
# memory (diffusers was not at hand to check them against): a correction is an edit of these two lines.  `LORA_KEY` is the name
# inside the bank; the checkpoint file carries it behind `LORA_FILE_PREFIX` (training_script.py:397-401).
LORA_KEY = "text_model.encoder.layers.{layer}.self_attn.{proj}.lora_linear_layer.{factor}.weight"
LORA_FILE_PREFIX = "text_encoder."


def lora_key(layer, proj, factor):
    """the bank's name of one factor: proj in PROJS, factor in ("down", "up")"""
    return LORA_KEY.format(layer=layer, proj=proj, factor=factor)


class ClipLoRABank(ops.LoRAStore):
    """The text tower's LoRA factors in the flat-buffer store of ops.LoRAStore: per layer one group (q_proj, k_proj, v_proj) -
    they read the same normed activation - and one group (out_proj), at scale 1.  `self.group[(layer, "qkv" | "out")]`."""

    def __init__(self, cfg: ClipTextConfig, lora_sd: dict, dtype, device):
        spec, keys = [], []
        for i in range(cfg.layers):
            for key, projs in (("qkv", PROJS[:3]), ("out", PROJS[3:])):
                members = []
                for p in projs:
                    dn, un = lora_key(i, p, "down"), lora_key(i, p, "up")
                    for n in (dn, un):
                        if n not in lora_sd:
                            raise KeyError(f"text-encoder LoRA state dict lacks {n}")
                    d, u = lora_sd[dn], lora_sd[un]
                    if d.dim() != 2 or d.shape[1] != cfg.hidden or tuple(u.shape) != (cfg.hidden, d.shape[0]):
                        raise ValueError(f"{dn} / {un}: shapes {tuple(d.shape)} / {tuple(u.shape)} do not fit hidden {cfg.hidden}")
                    members.append((dn, un, d, u))
                spec.append(members)
                keys.append((i, key))
        super().__init__(spec, dtype, device, scale=1.0)
        self.cfg = cfg
        self.group = dict(zip(keys, self.groups))

    @staticmethod
    def init(cfg: ClipTextConfig, rank: int, generator=None) -> dict:
        """the reference's initial factors (diffusers' LoRALinearLayer): down ~ N(0, 1/rank), up = 0"""
        sd = {}
        for i in range(cfg.layers):
            for p in PROJS:
                sd[lora_key(i, p, "down")] = torch.randn(rank, cfg.hidden, generator=generator) / rank
                sd[lora_key(i, p, "up")] = torch.zeros(cfg.hidden, rank)
        return sd


TEXT_PREFIX = "text_model."
TOK_NAME, POS_NAME = "embeddings.token_embedding.weight", "embeddings.position_embedding.weight"


def text_param_shapes(cfg: ClipTextConfig) -> dict:
    """name (without the text_model. prefix) -> shape of every parameter of CLIPTextModel, in the model's order"""
    d, out = cfg.hidden, {TOK_NAME: (cfg.vocab_size, cfg.hidden), POS_NAME: (cfg.max_pos, cfg.hidden)}

    def lin(name, n_out, n_in):
        out[name + ".weight"], out[name + ".bias"] = (n_out, n_in), (n_out,)

    for i in range(cfg.layers):
        L = f"encoder.layers.{i}."
        for p in ("k_proj", "v_proj", "q_proj", "out_proj"):
            lin(L + "self_attn." + p, d, d)
        lin(L + "layer_norm1", d, None)
        lin(L + "mlp.fc1", cfg.mlp, d)
        lin(L + "mlp.fc2", d, cfg.mlp)
        lin(L + "layer_norm2", d, None)
    lin("final_layer_norm", d, None)
    return {n: tuple(x for x in shp if x is not None) for n, shp in out.items()}


class ClipTextBank:
    """Every parameter of the text tower under `--tune_text_encoder` (training_utils/pipeline.py:69 `text_encoder.requires_grad_`,
    :173-174 its parameters join the generator's optimizer; training_script.py:304-305 keeps the tower fp32): every floating-point
    entry of the `CLIPTextModel` state dict in ONE flat fp32 master `flat` and ONE flat gradient `flat_grad`, the analogue of
    unet.UNetBank for the tower.
      * keys: transformers' names, with or without the `text_model.` prefix; `state_dict()` gives back the spelling that was
        loaded.  `embeddings.position_ids` (a buffer of some transformers versions) and other non-floating entries are ignored;
      * the Linear weights (2-D entries other than the two tables) have a compute-dtype copy in `flat_c` (only they: in fp32 the
        master is the copy) and a transpose in `flat_t`, rewritten from the master by ONE comat_weights_refresh launch in
        ensure_compute_copy() after an update (refresh.RefreshPlan);
      * biases, LayerNorm parameters and the two tables are read from the master: the embedding forward sums the fp32 rows and rounds
        once (ops.trained_embedding), so the 38 M-element token table of CLIP ViT-L has no second copy and nothing to refresh;
      * `gate`, `epoch`, zero_grad / set_requires_grad / mark_updated / ensure_compute_copy: UNetBank's protocol, what the training
        step asks of a bank.
    Every parameter starts on a 32-byte boundary (pad elements are zero and stay zero under AdamW).  `params[name]` is a leaf view
    whose .grad is a view of the flat gradient; names are the ones without the prefix."""

    def __init__(self, cfg: ClipTextConfig, sd: dict, dtype=torch.bfloat16, device="cuda"):
        self.cfg, self.dtype, self.device = cfg, dtype, device
        shapes = text_param_shapes(cfg)
        self.keys = {}  # name -> the key it was loaded under
        for key, t in sd.items():
            name = key[len(TEXT_PREFIX):] if key.startswith(TEXT_PREFIX) else key
            if not torch.is_tensor(t) or not t.is_floating_point() or name.endswith("position_ids"):
                continue
            if name not in shapes:
                raise KeyError(f"CLIP text state dict: {key} is not a parameter of the {cfg.layers}-layer text tower")
            self.keys[name] = key
        self.names = [n for n in shapes if n in self.keys]
        self._check(sd, self.keys, shapes)
        r8 = lambda n: -(-n // 8) * 8
        self.layout, self._coff, off, coff = {}, {}, 0, 0  # _coff: a Linear weight's place in flat_c and in flat_t
        for n in self.names:
            shp = shapes[n]
            numel = shp[0] * (shp[1] if len(shp) == 2 else 1)
            self.layout[n] = (off, shp)
            off += r8(numel)
            if len(shp) == 2 and n not in (TOK_NAME, POS_NAME):
                self._coff[n] = coff
                coff += r8(numel)
        self.flat = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_grad = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_c = None if dtype == torch.float32 else torch.zeros(coff, dtype=dtype, device=device)
        self.flat_t = torch.zeros(coff, dtype=dtype, device=device)
        self.gate = torch.zeros(1, dtype=torch.float32, device=device, requires_grad=True)
        self.params, self.holders, self._affine, self._made = {}, [], [], {}
        for n in self.names:
            p = self._view(self.flat, n).requires_grad_(True)
            p.grad = self._view(self.flat_grad, n)
            self.params[n] = p
        self._problems, self._plan = [], None
        self._fresh, self.epoch, self.training = False, 0, True
        self.load_state_dict(sd)

    @staticmethod
    def _check(sd, keys, shapes):
        """keys: name -> the key of `sd` that holds it"""
        missing = [n for n in shapes if n not in keys]
        if missing:
            raise KeyError(f"CLIP text state dict lacks {len(missing)} entries: {missing[:3]}"
                           f"{'...' if len(missing) > 3 else ''} (looked for with and without the {TEXT_PREFIX} prefix)")
        for n, shp in shapes.items():
            got = tuple(sd[keys[n]].shape)
            if got != shp:
                raise ValueError(f"CLIP text state dict: {keys[n]} has shape {got}, the bank holds {shp}")

    def _view(self, buf, name):
        o, shp = self.layout[name]
        return buf[o:o + (shp[0] * (shp[1] if len(shp) == 2 else 1))].view(shp)

    def load_state_dict(self, sd):
        """copies every entry of a transformers-named state dict into the existing buffers; either key spelling is taken, whatever
        the bank was built from; a missing key or another shape is refused by name (training_script.py:189-190 `text_encoder.pt`)"""
        found = {}
        for n in self.names:
            for key in (n, TEXT_PREFIX + n):
                if key in sd:
                    found[n] = key
        self._check(sd, found, {n: self.layout[n][1] for n in self.names})
        with torch.no_grad():
            for n in self.names:
                self._view(self.flat, n).copy_(sd[found[n]].detach().float().to(self.device))
        self.mark_updated()

    def state_dict(self):
        """every floating-point entry under the key it was loaded with (fp32, CPU): loads into a stock CLIPTextModel by
        load_state_dict (training_script.py:405-406 `text_encoder.pt`)"""
        return {self.keys[n]: self._view(self.flat, n).detach().to("cpu", torch.float32).contiguous() for n in self.names}

    # ---- what the tower's layers are built from --------------------------------------------------------------------------------
    def _hold(self, name, make):
        h = self._made.get(name)
        if h is None:
            h, problems = make()
            h.gate, h.requires_grad = self.gate, self.training
            self.holders.append(h)
            self._problems += problems
            self._plan, self._fresh = None, False  # the new holder's copies have not been written yet
            self._made[name] = h
        return h

    def linear(self, name):
        def make():
            wn, bn = name + ".weight", name + ".bias"
            o, oc = self.layout[wn][0], self._coff[wn]
            N, K = self.layout[wn][1]
            if self.flat_c is None:  # fp32: the master is the forward copy (the refresh launch leaves it alone)
                w, ow = self._view(self.flat, wn), o
            else:
                w, ow = self.flat_c[oc:oc + N * K].view(N, K), oc
            return (ops.TrainableLinear(w, self._view(self.flat_grad, wn), self._view(self.flat, bn), self._view(self.flat_grad, bn),
                                        wt=self.flat_t[oc:oc + N * K].view(K, N)), refresh.linear_problem(o, ow, oc, N, K))
        return self._hold(name, make)

    def embedding(self):
        return self._hold("embeddings", lambda: (ops.TrainableEmbedding(
            self._view(self.flat, TOK_NAME), self._view(self.flat_grad, TOK_NAME), self._view(self.flat, POS_NAME),
            self._view(self.flat_grad, POS_NAME)), []))

    def norm(self, name):
        if name not in self._made:
            out = []
            for leaf in (".weight", ".bias"):
                t = self._view(self.flat, name + leaf)
                t.comat_grad, t.comat_train = self._view(self.flat_grad, name + leaf), self.training
                self._affine.append(t)
                out.append(t)
            self._made[name] = tuple(out)
        return self._made[name]

    # ---- the bank protocol of the training step ----------------------------------------------------------------------------------
    def ensure_compute_copy(self):
        if not self._fresh:
            if self._problems:
                if self._plan is None:  # built once the holders exist; the launch only reads it
                    self._plan = refresh.RefreshPlan(self._problems, self.device)
                self._plan.run(self.flat, self.flat_c, self.flat_t)
            self._fresh = True
            self.epoch += 1

    def mark_updated(self):
        """call after an in-place update of `flat` (optimizer kernel, load): the derived copies are refreshed lazily"""
        self._fresh = False

    def zero_grad(self):
        self.flat_grad.zero_()

    def set_requires_grad(self, flag: bool):
        self.training = bool(flag)
        self.gate.requires_grad_(self.training)
        for h in self.holders:
            h.requires_grad = self.training
        for t in self._affine:
            t.comat_train = self.training


class ClipTextEncoder:
    """`CLIPTextModel` under transformers' state-dict names, with or without the `text_model.` prefix (4.31 and the diffusers
    checkpoints carry it, 5.x does not); `embeddings.position_ids` is ignored.  bank: a ClipLoRABank, None (frozen tower) or a
    ClipTextBank (the tower trained in full: every layer reads the bank's parameters, `sd` is not read and may be None)."""

    def __init__(self, cfg: ClipTextConfig, sd: dict | None, dtype=torch.bfloat16, device="cuda",
                 bank: "ClipLoRABank | ClipTextBank | None" = None):
        self.cfg, self.dtype, self.device, self.bank = cfg, dtype, device, bank
        self.full = isinstance(bank, ClipTextBank)
        self.act = ops.quick_gelu if cfg.act == "quick_gelu" else ops.gelu
        if self.full:
            if bank.dtype != dtype or torch.device(bank.device) != torch.device(device) or bank.cfg != cfg:
                raise ValueError("ClipTextEncoder: the bank was built for another config, dtype or device")
            self._from_bank(bank)
            return
        d = cfg.hidden

        def get(name, shape):
            for key in (name, "text_model." + name):
                if key in sd:
                    if tuple(sd[key].shape) != tuple(shape):
                        raise ValueError(f"{key}: shape {tuple(sd[key].shape)}, the config needs {tuple(shape)}")
                    return sd[key]
            raise KeyError(f"CLIP text state dict lacks {name} (looked for it with and without the text_model. prefix)")

        def lin(name, n_out, n_in):
            return ops.FrozenLinear(get(name + ".weight", (n_out, n_in)), get(name + ".bias", (n_out,)), dtype, device)

        def norm(name):
            f = lambda t: t.to(device=device, dtype=torch.float32).contiguous()
            return f(get(name + ".weight", (d,))), f(get(name + ".bias", (d,)))

        f = lambda t: t.to(device=device, dtype=dtype).contiguous()
        self.tok = f(get("embeddings.token_embedding.weight", (cfg.vocab_size, d)))
        self.pos = f(get("embeddings.position_embedding.weight", (cfg.max_pos, d)))
        self.layers = []
        for i in range(cfg.layers):
            L = f"encoder.layers.{i}."
            self.layers.append(dict(
                ln1=norm(L + "layer_norm1"), qkv=tuple(lin(L + "self_attn." + p, d, d) for p in PROJS[:3]),
                out=lin(L + "self_attn.out_proj", d, d), ln2=norm(L + "layer_norm2"),
                fc1=lin(L + "mlp.fc1", cfg.mlp, d), fc2=lin(L + "mlp.fc2", d, cfg.mlp)))
        self.final_ln = norm("final_layer_norm")

    def _from_bank(self, bank):
        """trained holders and norms of a ClipTextBank; the embedding is the fused node over the master tables"""
        self.emb = bank.embedding()
        self.layers = []
        for i in range(self.cfg.layers):
            L = f"encoder.layers.{i}."
            self.layers.append(dict(
                ln1=bank.norm(L + "layer_norm1"), qkv=tuple(bank.linear(L + "self_attn." + p) for p in PROJS[:3]),
                out=bank.linear(L + "self_attn.out_proj"), ln2=bank.norm(L + "layer_norm2"),
                fc1=bank.linear(L + "mlp.fc1"), fc2=bank.linear(L + "mlp.fc2")))
        self.final_ln = bank.norm("final_layer_norm")

    def __call__(self, input_ids, output="last"):
        """input_ids [B, L] -> tokens [B*L, hidden] in the package's row layout.  "last": final_layer_norm of the last layer
        (`last_hidden_state`); "penultimate": `hidden_states[-2]`, the input of the last layer, without the final norm."""
        if output not in ("last", "penultimate"):
            raise ValueError(f"output must be 'last' or 'penultimate', got {output!r}")
        cfg = self.cfg
        B, L = input_ids.shape
        if L > cfg.max_pos:
            raise ValueError(f"{L} tokens, the position table has {cfg.max_pos}")
        d, nh = cfg.hidden, cfg.heads
        lora = self.bank is not None and not self.full
        grp = (lambda i, key: self.bank.group[(i, key)]) if lora else (lambda i, key: None)
        if self.full:
            self.bank.ensure_compute_copy()
            h = ops.trained_embedding(input_ids.to(self.device).reshape(-1), self.emb, L, self.dtype)
        else:
            h = ops.embedding(input_ids.to(self.device).reshape(-1), self.tok)
            h = ops.add_rowvec(h.reshape(B, L * d), self.pos[:L].reshape(-1)).reshape(B * L, d)
        for i, Lr in enumerate(self.layers):
            if output == "penultimate" and i == cfg.layers - 1:
                return h
            x, h = ops.layer_norm_fork(h, *Lr["ln1"], eps=cfg.eps)
            q, k, v = ops.lora_group_linear(x, Lr["qkv"], grp(i, "qkv"))
            o, _ = ops.attention(q, k, v, B, L, L, nh, d // nh, causal=True)
            h = ops.lora_linear(o, Lr["out"], grp(i, "out"), residual=h)
            x, h = ops.layer_norm_fork(h, *Lr["ln2"], eps=cfg.eps)
            h = ops.linear(self.act(ops.linear(x, Lr["fc1"])), Lr["fc2"], residual=h)
        return ops.layer_norm(h, *self.final_ln, eps=cfg.eps)
