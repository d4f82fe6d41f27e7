"""Checkpoint wire format of the hot path: what `Trainer.save_model_hook`
(training_script.py:390-426) writes and `load_model_hook` (:170-196) reads, so adapters trained here load into a stock
diffusers pipeline (`pipe.load_lora_weights(dir)`) and adapters trained by the reference resume here.

    {dir}/pytorch_lora_weights.safetensors     keys  unet.{attention path}.{to_q|to_k|to_v|to_out.0}.lora.{down|up}.weight
                                               (unet_lora_state_dict, training_script.py:49-64; written by
                                               LoraLoaderMixin.save_lora_weights, safetensors, metadata format=pt)
                                               with `text=` (--train_text_encoder_lora) the SAME file also holds the text tower's
                                               factors, keys  text_encoder.text_model.encoder.layers.{i}.self_attn.
                                               {q|k|v|out}_proj.lora_linear_layer.{down|up}.weight
                                               (text_encoder_lora_state_dict, training_script.py:397-401; read back at :182-185;
                                               the names are one table in clip.py)
    {dir}/D_sd/pytorch_lora_weights.safetensors   the discriminator UNet's LoRA factors, same key scheme (:413-424)
    {dir}/D_sd/mlp.pt                          torch.save(nn.Sequential(nn.Linear(4, 1)).state_dict())  (:426;
                                               gan_sdxl.py:32-35) -> keys "0.weight" [1, 4], "0.bias" [1];
                                               with --gan_unet_lastlayer_cls the head is nn.Conv2d(C, 1, 3, padding=1)
                                               (gan_sdxl.py:27-30; :196-200) -> keys "weight" [1, C, 3, 3], "bias" [1]
    {dir}/vae.pt                               only with `vae=` (--tune_vae): torch.save(vae.state_dict()) (:402-403; read back
                                               at :187-188) - diffusers names, OIHW conv weights, every key of the VAE
    {dir}/unet.pt                              INSTEAD of the generator's LoRA file when `bank` is a unet.UNetBank (--full_finetuning):
                                               torch.save(unet.state_dict()) (:392-395; read back at :177-178) - diffusers names,
                                               OIHW conv weights, original row order, every key of the UNet
    {dir}/text_encoder.pt                      only with `text=` a clip.ClipTextBank (--tune_text_encoder): torch.save(
                                               text_encoder.state_dict()) (:405-406; read back at :189-190) - transformers names
                                               in the spelling the bank was loaded with, fp32, every floating-point entry
    {dir}/fp8_state.pt                         only with `fp8_device=`: ops.fp8_state_dict (this project's fp8 forward; no
                                               reference counterpart)
    {dir}/optim_state.pt                       only with `optim=`: {name: FlatAdamW.state_dict()} on the CPU - moments, the
                                               (applied, skipped) counters and the learning-rate schedule's fields.  A
                                               deliberate extension like fp8_state.pt: the reference saves no optimizer state,
                                               and after its resume the moments and the scheduler restart from zero

Frozen base weights are not part of a checkpoint; `load_safetensors` reads the upstream repositories' own files
(`unet/diffusion_pytorch_model.safetensors`, `vae/...`, BLIP `model.safetensors`): the model classes of this package
take those state dicts under their upstream names.
"""
from __future__ import annotations

import os

import torch
from safetensors.torch import load_file, save_file

LORA_WEIGHT_NAME = "pytorch_lora_weights.safetensors"
PREFIX = "unet."
FP8_STATE_NAME = "fp8_state.pt"
OPTIM_STATE_NAME = "optim_state.pt"


def lora_state_dict(bank) -> dict:
    """{'unet.<module>.lora.down.weight': fp32 CPU tensor, ...} in the bank's parameter order."""
    return {PREFIX + n: p.detach().to("cpu", torch.float32).contiguous() for n, p in bank.params.items()}


def text_lora_state_dict(text_bank) -> dict:
    """{'text_encoder.<clip.LORA_KEY name>': fp32 CPU tensor, ...} in the text bank's parameter order"""
    from .clip import LORA_FILE_PREFIX
    return {LORA_FILE_PREFIX + n: p.detach().to("cpu", torch.float32).contiguous() for n, p in text_bank.params.items()}


def save_lora_weights(save_directory: str, bank, weight_name: str = LORA_WEIGHT_NAME, text=None) -> str:
    """text: a clip.ClipLoRABank whose factors go into the same file (training_script.py:397-401); None: the UNet's alone"""
    os.makedirs(save_directory, exist_ok=True)
    path = os.path.join(save_directory, weight_name)
    sd = lora_state_dict(bank)
    if text is not None:
        sd.update(text_lora_state_dict(text))
    save_file(sd, path, metadata={"format": "pt"})
    return path


def load_lora_state_dict(path: str) -> dict:
    """Reads a LoRA safetensors file (or the directory holding `pytorch_lora_weights.safetensors`) and returns the
    UNet factors keyed WITHOUT the 'unet.' prefix (the key scheme of LoRABank / weights.make_lora_weights).
    Text-encoder LoRA entries (prefix 'text_encoder.') are read by load_text_lora_into_bank and ignored here."""
    if os.path.isdir(path):
        path = os.path.join(path, LORA_WEIGHT_NAME)
    sd = load_file(path)
    return {k[len(PREFIX):]: v.float() for k, v in sd.items() if k.startswith(PREFIX)}


def load_text_lora_into_bank(text_bank, path: str):
    """Copies the file's text-encoder factors (prefix 'text_encoder.', training_script.py:182-185) into the text bank's flat fp32
    buffer.  A file that lacks one of the bank's factors, or holds it in another shape, is refused, naming the key."""
    from .clip import LORA_FILE_PREFIX
    if os.path.isdir(path):
        path = os.path.join(path, LORA_WEIGHT_NAME)
    sd = load_file(path)
    for n, p in text_bank.params.items():
        key = LORA_FILE_PREFIX + n
        if key not in sd:
            raise KeyError(f"{path} lacks the text-encoder LoRA factor {key}")
        if tuple(sd[key].shape) != tuple(p.shape):
            raise ValueError(f"{key}: shape {tuple(sd[key].shape)} != {tuple(p.shape)}")
    extra = [k for k in sd if k.startswith(LORA_FILE_PREFIX) and k[len(LORA_FILE_PREFIX):] not in text_bank.params]
    if extra:
        raise KeyError(f"{path} holds text-encoder LoRA factors the bank does not have: {extra[:3]}...")
    with torch.no_grad():
        for n, p in text_bank.params.items():
            p.copy_(sd[LORA_FILE_PREFIX + n].to(p.device, torch.float32))
    text_bank.mark_updated()


def load_lora_into_bank(bank, sd: dict):
    """Copies factors into the bank's flat fp32 buffer (shapes and names must match: same rank, same attention set)."""
    missing = [n for n in bank.names if n not in sd]
    extra = [n for n in sd if n not in bank.params]
    if missing or extra:
        raise KeyError(f"LoRA state dict does not match the bank: missing {missing[:3]}..., unexpected {extra[:3]}...")
    with torch.no_grad():
        for n, p in bank.params.items():
            if tuple(sd[n].shape) != tuple(p.shape):
                raise ValueError(f"{n}: shape {tuple(sd[n].shape)} != {tuple(p.shape)}")
            p.copy_(sd[n].to(p.device, torch.float32))
    bank.mark_updated()


VAE_WEIGHT_NAME = "vae.pt"  # the files of the banks trained in full, as the banks name them (MasterBank.weight_file)
UNET_WEIGHT_NAME = "unet.pt"
TEXT_WEIGHT_NAME = "text_encoder.pt"


def _weight_file(bank):
    """the file that holds the state dict of a bank trained in full (bank.MasterBank.weight_file); None for a LoRA store"""
    return getattr(bank, "weight_file", None)


def save_checkpoint(output_dir: str, bank, disc=None, fp8_device=None, optim=None, vae=None, text=None):
    """training_script.py:390-426 (frozen text encoder).  bank: the generator's LoRABank, or its unet.UNetBank under
    `--full_finetuning` - then {dir}/unet.pt is written instead of the LoRA file (:392-395).
    fp8_device: also write {dir}/fp8_state.pt, the delayed-scaling state of that device (ops.fp8_state_dict: scales, abs-max
    history, clip accounting, recipe) - a resumed run then continues under the same scales.  None: the files above only.
    optim: a dict of optimizers (step.FlatAdamW), e.g. dict(G=trainer.opt, D=trainer.opt_D): also write {dir}/optim_state.pt,
    their moments, counters and learning-rate schedules, so that a resumed run continues the schedule where it stopped.  A
    deliberate extension, like fp8_state.pt: the reference saves no optimizer state, and after its resume the scheduler
    restarts from zero.  None: the files are exactly those of the reference.
    vae: the unet.VAEBank of a `--tune_vae` run: also write {dir}/vae.pt (training_script.py:402-403 `torch.save(vae.state_dict())`):
    a torch.save'd state dict under diffusers names with OIHW conv weights, every key of the state dict the decoder was built
    from (encoder entries as they came); a stock AutoencoderKL loads it by load_state_dict (:187-188).
    text: the clip.ClipLoRABank of a `--train_text_encoder_lora` run: its factors go into the generator's LoRA file under the
    `text_encoder.` prefix (:397-401).  None: that file is byte for byte what it is without the argument.  The clip.ClipTextBank
    of a `--tune_text_encoder` run instead: {dir}/text_encoder.pt (:405-406 `torch.save(text_encoder.state_dict())`), the bank's
    state dict, fp32, under the key spelling it was loaded with - with a LoRABank or a UNetBank; the LoRA file carries nothing of it."""
    if _weight_file(text):
        os.makedirs(output_dir, exist_ok=True)
        torch.save(text.state_dict(), os.path.join(output_dir, text.weight_file))
        text = None
    if text is not None and _weight_file(bank):
        raise ValueError("text= with a UNetBank: full_finetuning writes no LoRA file that could hold the text factors")
    if _weight_file(bank):  # --full_finetuning (:392-395): the whole UNet's state dict, and no LoRA file for the generator
        os.makedirs(output_dir, exist_ok=True)
        torch.save(bank.state_dict(), os.path.join(output_dir, bank.weight_file))
    else:
        save_lora_weights(output_dir, bank, text=text)
    if vae is not None:
        torch.save(vae.state_dict(), os.path.join(output_dir, vae.weight_file))
    if disc is not None:
        d = os.path.join(output_dir, "D_sd")
        save_lora_weights(d, disc.bank)
        torch.save(disc.head_state_dict(), os.path.join(d, "mlp.pt"))
    if fp8_device is not None:
        from . import ops
        torch.save(ops.fp8_state_dict(fp8_device), os.path.join(output_dir, FP8_STATE_NAME))
    if optim is not None:
        to_cpu = lambda v: v.cpu() if torch.is_tensor(v) else [t.cpu() for t in v] if isinstance(v, list) else v
        torch.save({name: {k: to_cpu(v) for k, v in opt.state_dict().items()} for name, opt in optim.items()},
                   os.path.join(output_dir, OPTIM_STATE_NAME))


def load_checkpoint(load_dir: str, bank, disc=None, fp8_device=None, optim=None, vae=None, text=None):
    """training_script.py:170-196; fp8_device: also restore {dir}/fp8_state.pt into that device's site tables (save_checkpoint);
    optim: the same dict of optimizers as at save_checkpoint - {dir}/optim_state.pt is copied INTO their buffers
    (FlatAdamW.load_state_dict: addresses stay, so captured graphs stay valid) and the learning-rate word is re-evaluated;
    vae: the unet.VAEBank of a `--tune_vae` run: {dir}/vae.pt is copied INTO its buffers (training_script.py:187-188); a file that
    lacks a decoder entry is refused (KeyError);
    text: the clip.ClipLoRABank of a `--train_text_encoder_lora` run: the `text_encoder.` entries of the generator's LoRA file are
    copied INTO its buffers (:182-185); a file that lacks one (KeyError) or holds another shape (ValueError) is refused.  The
    clip.ClipTextBank of a `--tune_text_encoder` run: {dir}/text_encoder.pt is copied INTO its buffers (:189-190), refused alike"""
    if _weight_file(bank):  # :177-178 `unet.load_state_dict(torch.load(unet.pt))`: a missing key or another shape is refused
        bank.load_state_dict(torch.load(os.path.join(load_dir, bank.weight_file), map_location="cpu"))
    else:
        load_lora_into_bank(bank, load_lora_state_dict(load_dir))
    if _weight_file(text):
        text.load_state_dict(torch.load(os.path.join(load_dir, text.weight_file), map_location="cpu"))
    elif text is not None:
        load_text_lora_into_bank(text, load_dir)
    if vae is not None:
        vae.load_state_dict(torch.load(os.path.join(load_dir, vae.weight_file), map_location="cpu"))
    if disc is not None:
        d = os.path.join(load_dir, "D_sd")
        load_lora_into_bank(disc.bank, load_lora_state_dict(d))
        # raises when the file holds the other head (a Linear file for a conv head or the reverse)
        disc.load_head_state_dict(torch.load(os.path.join(d, "mlp.pt"), map_location="cpu"))
    if fp8_device is not None:
        from . import ops
        ops.fp8_load_state_dict(fp8_device, torch.load(os.path.join(load_dir, FP8_STATE_NAME), map_location="cpu"))
    if optim is not None:
        sd = torch.load(os.path.join(load_dir, OPTIM_STATE_NAME), map_location="cpu")
        if set(sd) != set(optim):
            raise KeyError(f"{OPTIM_STATE_NAME} holds the optimizers {sorted(sd)}, asked for {sorted(optim)}")
        for name, opt in optim.items():
            opt.load_state_dict(sd[name])


def load_safetensors(path: str) -> dict:
    """Frozen base weights under their upstream names (e.g. runwayml/stable-diffusion-v1-5
    unet/diffusion_pytorch_model.safetensors, Salesforce/blip-image-captioning-large model.safetensors)."""
    return load_file(path)
