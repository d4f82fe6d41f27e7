"""CLIP text tower on the HIP operators, with trainable LoRA on its attention projections (--train_text_encoder_lora) or trained in
full (--tune_text_encoder: `ClipTextBank`).

Mirrors transformers' `CLIPTextModel` forward as the reference calls it (`TrainableSDPipeline.py:325-326`:
`text_encoder(ids, attention_mask=None)[0]`): token + position embedding, pre-LN blocks (layer_norm1 -> q / k / v with bias ->
causal self-attention -> out_proj -> residual; layer_norm2 -> fc1 -> quick-GELU -> fc2 -> residual) and the final layer norm.
The causal mask is the only mask: the reference passes no key-padding mask.  The frozen weights carry no gradient, the ids carry
none; the LoRA factors of a `ClipLoRABank` do (`LoraLoaderMixin._modify_text_encoder`, training_utils/pipeline.py:117-119,176-184:
fp32 LoRA on q_proj / k_proj / v_proj / out_proj of every layer at scale 1, the MLP left alone - `patch_mlp` defaults to False).
Tokenisation stays outside: the encoder takes input ids.

With `ClipTextConfig.projection_dim` set the tower is transformers' `CLIPTextModelWithProjection` - SDXL's `pipeline.text_encoder_2`
(config.CLIP_BIGG_TEXT: erf-GELU, a bias-free `text_projection`), frozen in the reference: `output="pooled"` gives hidden_states[-2]
and `text_embeds` from one pass (ops.eos_pool: the end token's row alone takes the final norm), and `encode_prompt_sdxl` joins the two
towers as diffusers' `StableDiffusionXLPipeline.encode_prompt` does.
"""
from __future__ import annotations

import torch

from . import ops
from .bank import MasterBank
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
PROJ_NAME = "text_projection.weight"  # CLIPTextModelWithProjection's bias-free Linear [projection_dim, hidden], outside text_model.


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


class ClipTextBank(MasterBank):
    """Every parameter of the text tower under `--tune_text_encoder` (training_utils/pipeline.py:69 `text_encoder.requires_grad_`,
    :173-174 its parameters join the generator's optimizer; training_script.py:304-305 keeps the tower fp32): every floating-point
    entry of the `CLIPTextModel` state dict in a bank.MasterBank, under its name without the `text_model.` prefix.  What the tower
    adds:
      * keys: transformers' names, with or without the prefix; `state_dict()` gives back the spelling that was loaded (`keys`).
        `embeddings.position_ids` (a buffer of some transformers versions) and other non-floating entries are ignored;
      * the two tables are no matrices of the bank: the embedding forward sums their fp32 master rows and rounds once
        (ops.trained_embedding, `embedding()`), so the 38 M-element token table of CLIP ViT-L has no second copy and nothing to
        refresh - and `flat_c` is compact: it holds the Linear weights only, at flat_t's offsets."""

    MODEL, weight_file = "CLIP text", "text_encoder.pt"

    def __init__(self, cfg: ClipTextConfig, sd: dict, dtype=torch.bfloat16, device="cuda"):
        self.cfg = cfg
        shapes = text_param_shapes(cfg)
        for key, t in sd.items():
            name = key[len(TEXT_PREFIX):] if key.startswith(TEXT_PREFIX) else key
            if torch.is_tensor(t) and t.is_floating_point() and not name.endswith("position_ids") and name not in shapes:
                raise KeyError(f"CLIP text state dict: {key} is not a parameter of the {cfg.layers}-layer text tower")
        super().__init__({n: (shp, shp) for n, shp in shapes.items()},
                         [n for n, shp in shapes.items() if len(shp) == 2 and n not in (TOK_NAME, POS_NAME)], dtype, device, compact=True)
        self.keys = self._keys_of(sd)  # name -> the key it was loaded under
        self.load_state_dict(sd)

    def _keys_of(self, sd):
        return {n: key for n in self.names for key in (n, TEXT_PREFIX + n) if key in sd}

    def _lacks(self, missing):
        return (f"CLIP text state dict lacks {len(missing)} entries: {missing[:3]}{'...' if len(missing) > 3 else ''} "
                f"(looked for with and without the {TEXT_PREFIX} prefix)")

    def state_dict(self):
        """every floating-point entry under the key it was loaded with (fp32, CPU): loads into a stock CLIPTextModel by
        load_state_dict (training_script.py:189-190,405-406 `text_encoder.pt`)"""
        return {self.keys[n]: t for n, t in super().state_dict().items()}

    def embedding(self):
        return self._once("embeddings", "embedding", lambda: (ops.TrainableEmbedding(
            self._view(self.flat, TOK_NAME), self._view(self.flat_grad, TOK_NAME), self._view(self.flat, POS_NAME),
            self._view(self.flat_grad, POS_NAME)), []))


class ClipTextEncoder:
    """`CLIPTextModel` under transformers' state-dict names, with or without the `text_model.` prefix (4.31 and the diffusers
    checkpoints carry it, 5.x does not); `embeddings.position_ids` is ignored.  bank: a ClipLoRABank, None (frozen tower) or a
    ClipTextBank (the tower trained in full: every layer reads the bank's parameters, `sd` is not read and may be None)."""

    def __init__(self, cfg: ClipTextConfig, sd: dict | None, dtype=torch.bfloat16, device="cuda",
                 bank: "ClipLoRABank | ClipTextBank | None" = None):
        self.cfg, self.dtype, self.device, self.bank = cfg, dtype, device, bank
        self.full = isinstance(bank, ClipTextBank)
        self.act = ops.quick_gelu if cfg.act == "quick_gelu" else ops.gelu
        self.proj = None
        if cfg.projection_dim is not None and bank is not None:
            # the reference trains `pipeline.text_encoder` only (training_utils/pipeline.py:119,173-174): the pooled row has no backward
            raise NotImplementedError("ClipTextEncoder: a bank (LoRA or full) on a tower with projection_dim is not built")
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
        if cfg.projection_dim is not None:  # CLIPTextModelWithProjection: the key sits beside `text_model.`, not under it
            if PROJ_NAME not in sd:
                raise KeyError(f"CLIP text state dict lacks {PROJ_NAME} (ClipTextConfig.projection_dim = {cfg.projection_dim})")
            if tuple(sd[PROJ_NAME].shape) != (cfg.projection_dim, d):
                raise ValueError(f"{PROJ_NAME}: shape {tuple(sd[PROJ_NAME].shape)}, the config needs {(cfg.projection_dim, d)}")
            self.proj = ops.FrozenLinear(sd[PROJ_NAME], None, dtype, device)

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
        (`last_hidden_state`); "penultimate": `hidden_states[-2]`, the input of the last layer, without the final norm.
        "pooled" (a tower with projection_dim): (hidden_states[-2] [B*L, hidden], text_embeds [B, projection_dim]) from ONE pass -
        the penultimate state is kept on the way, the last layer runs, the end token's row alone takes the final norm
        (ops.eos_pool) and the bias-free text_projection: CLIPTextModelWithProjection's `text_embeds`."""
        if output not in ("last", "penultimate", "pooled"):
            raise ValueError(f"output must be 'last', 'penultimate' or 'pooled', got {output!r}")
        if output == "pooled" and self.proj is None:
            raise ValueError("output='pooled' needs a tower with a text_projection (ClipTextConfig.projection_dim is None)")
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
        penultimate = None
        for i, Lr in enumerate(self.layers):
            if i == cfg.layers - 1:
                if output == "penultimate":
                    return h
                penultimate = h
            x, h = ops.layer_norm_fork(h, *Lr["ln1"], eps=cfg.eps)
            q, k, v = ops.lora_group_linear(x, Lr["qkv"], grp(i, "qkv"))
            o, _ = ops.attention(q, k, v, B, L, L, nh, d // nh, causal=True, need_probs=False)
            h = ops.lora_linear(o, Lr["out"], grp(i, "out"), residual=h)
            x, h = ops.layer_norm_fork(h, *Lr["ln2"], eps=cfg.eps)
            h = ops.linear(self.act(ops.linear(x, Lr["fc1"])), Lr["fc2"], residual=h)
        if output == "pooled":
            pooled = ops.eos_pool(input_ids.to(self.device), h, *self.final_ln, L, cfg.eos_token_id, eps=cfg.eps)
            return penultimate, ops.linear(pooled, self.proj)
        return ops.layer_norm(h, *self.final_ln, eps=cfg.eps)


def encode_prompt_sdxl(enc1: ClipTextEncoder, enc2: ClipTextEncoder, ids_1, ids_2):
    """diffusers' StableDiffusionXLPipeline.encode_prompt for one list of prompts, clip_skip=None, no guidance, as the reference
    calls it for the null prompt and the discriminator's conditioning (training_script.py:516,523; gan_sdxl.py:298-302):
    -> (prompt_embeds [B, L, hidden1 + hidden2] = [enc1.hidden_states[-2] | enc2.hidden_states[-2]] along the channels,
        pooled [B, projection_dim] = the SECOND tower's text_embeds).
    ids_1 / ids_2 [B, L]: the two tokenizers' ids of the same prompts.  enc2 is frozen (no bank) and runs without autograd; enc1's
    gradient passes through the concat where it carries a bank.  Under no_grad the whole is preprocessing: the GT-latent producer,
    gan_null_embeds / gan_pooled_null_embeds."""
    if enc2.proj is None:
        raise ValueError("encode_prompt_sdxl: the second tower has no text_projection (ClipTextConfig.projection_dim is None)")
    if tuple(ids_1.shape) != tuple(ids_2.shape):
        raise ValueError(f"encode_prompt_sdxl: ids_1 {tuple(ids_1.shape)} and ids_2 {tuple(ids_2.shape)} differ in shape")
    if enc1.dtype != enc2.dtype:
        raise ValueError(f"encode_prompt_sdxl: the towers compute in {enc1.dtype} and {enc2.dtype}")
    B, L = ids_1.shape
    e1 = enc1(ids_1, output="penultimate")
    with torch.no_grad():
        e2, pooled = enc2(ids_2, output="pooled")
    return ops.concat_cols(e1, e2).reshape(B, L, -1), pooled
