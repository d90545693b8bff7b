"""``Jen1``: the top-level generate() surface of the reference around the HIP denoiser path.

Host-side mirror of /root/reference/generation.py:16-192 -- same constructor arguments, ``get_model_and_diffusion``,
``generate(prompt, seed, steps, batch_size, seconds, use_gdm, task, init_audio, init_audio_sr, inpainting_scope)`` (plus the keyword
additions ``sampler``, ``preserve_known``, ``output_sr`` and ``normalize`` / ``target_lufs`` / ``limit`` with ``ceiling_dbtp`` / ``lookahead_ms`` / ``release_ms``),``get_mask``, ``get_emb``, ``get_conditioning`` -- with the two third-party models the reference constructs itself
passed in instead (their weights are outside this build):

  * ``audio_encoder``: the object the reference gets from ``EncodecModel.encodec_model_48khz()``; used exactly as
    generation.py uses it: ``.channels``, ``.encode(audio) -> [(codes, scale)]``, ``.quantizer.decode(codes)``,
    ``.decoder(emb)``  (generation.py:34, :95, :113, :130, :145-150);
  * ``conditioner``: the ``MultiConditioner`` of ``create_multi_conditioner`` (generation.py:29, :121-122),
    ``conditioner(batch_metadata, device) -> {"prompt": (emb [B,128,1024], mask [B,128])}``.  ``jen1_amd.t5.T5ConditionerHIP`` is one: the
    reference's ``T5Conditioner`` with the T5 encoder stack and ``proj_out`` on the HIP path (csrc/t5.hip); it takes the caller's tokenizer
    and the encoder's ``state_dict`` (the checkpoint itself is not part of this build);
  * ``convert_audio``: ``encodec.utils.convert_audio`` (generation.py:95).  Optional: the default is ``jen1_amd.audio.convert_audio``, the
    same channel rule and windowed-sinc resampler as one HIP kernel on ``device`` (csrc/audio.hip).  Audio that already has the model's
    sample rate and channel count is passed through untouched, without loading the library.

Everything between them -- the masks, the conditioning dict, the 100-step DDIM loop over the UNet with the CFG pair,
captured as one HIP graph per shape -- runs on libjen1_hip.so through ``GaussianDiffusion.sample``; ``generate(output_sr=...)`` resamples
the decoder's output with the kernel of ``convert_audio``.

Differences, all deliberate and visible:
  * ``use_gdm=False`` (the reference default) selects ``VDM``, which cannot run in the reference (SURVEY.md Appendix
    A-3 / A-4); here it runs the REPAIRED sampler of jen1_amd/vdm.py (same formulas, the three repairs listed there).  The
    reference also passes ``causal`` positionally into VDM.sample's ``step`` slot (generation.py:128 vs vdm.py:77), which would
    run zero steps; ``steps`` and ``causal`` go to their own parameters here;
  * the reference reads ``flag`` before assignment when ``init_audio`` is given (generation.py:91-120); here
    ``flag`` is False in that case, i.e. the given audio is the ``init_data`` of the sampler, which is what the code
    evidently means;
  * ``init_audio.size() != 3`` (generation.py:85) compares a ``torch.Size`` with an int and is always true, so the
    reference repeats even batched audio ``batch_size`` times; here only audio without a batch axis is repeated;
  * ``music_cont`` appends ``randn * mask[:, cont_start:]`` to the prefix (generation.py:105-107; the slice is on the
    size-1 channel axis); the mask is 0 over the whole extension and the extension is multiplied by the mask again before it
    reaches the network, so zeros are appended here (no noise draw: the sampler's own draws start at the same generator state
    only if the reference's draw is skipped too -- the test compares against the hand-built call, not a bit-stream);
  * the decoder gets the latents on its own device (``audio_encoder.decoder_device``, default "cpu" as in
    generation.py:129): with ``EncodecHIP`` they never leave HBM.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from .checkpoint import load_checkpoint, load_normalizer
from .config import GDMConfig, VDMConfig, full_model_config
from .diffusion import GaussianDiffusion, get_beta_schedule
from .model import UNetCFG1d
from .tasks import get_conditioning, get_mask


def known_segment_scales(scales: torch.Tensor, keep: torch.Tensor, segments: Sequence[Tuple[int, int]]) -> torch.Tensor:
    """the ``segment_scales="known"`` policy of ``Jen1.generate``: ``scales`` [B, S] are the encoder's per-segment scales of the known
    audio, ``keep`` the sample mask (1 = kept; [N], or [B, 1, N] as ``get_mask`` returns it, the same for every batch element),
    ``segments`` the (offset, samples) of every segment.  A segment lying wholly inside the kept region keeps its own scale; every other
    segment gets the RMS of those scales, ``sqrt(mean(scale^2))`` per batch element, and 1.0 when no segment is wholly kept."""
    scales = torch.as_tensor(scales, dtype=torch.float32)
    k = torch.as_tensor(keep).reshape(-1, keep.shape[-1])[0] != 0
    if scales.dim() != 2 or scales.shape[1] != len(segments):
        raise ValueError(f"scales {tuple(scales.shape)} do not match the {len(segments)} segments")
    kept = torch.tensor([bool(n > 0 and k[off:off + n].numel() == n and k[off:off + n].all()) for off, n in segments], device=scales.device)
    if not bool(kept.any()):
        return torch.ones_like(scales)
    fill = scales[:, kept].pow(2).mean(dim=1, keepdim=True).sqrt()
    return torch.where(kept[None, :], scales, fill.expand_as(scales))


class Jen1:
    def __init__(self, ckpt_path: Optional[str], device: str = "cuda", sample_rate: int = 48000,
                 cross_attn_cond_ids: Sequence[str] = ("prompt",), global_cond_ids: Sequence[str] = (),
                 input_concat_ids: Sequence[str] = ("masked_input", "mask"), *, audio_encoder, conditioner: Callable,
                 convert_audio: Optional[Callable] = None, model_config: Optional[dict] = None,
                 diffusion_config: Optional[GDMConfig] = None, compute_dtype: str = "bf16", vdm_config: Optional[VDMConfig] = None,
                 weights: str = "model", latents: str = "codes", normalizer=None):
        """``weights="ema"`` (keyword-only, not in the reference): sample from the checkpoint's EMA weights (``checkpoint.load_checkpoint``).
        ``latents`` (keyword-only, not in the reference): ``"codes"`` builds the known latents as generation.py:145-150 does, ``encode`` then
        ``quantizer.decode`` of the concatenated codes; ``"fused"`` asks ``audio_encoder.encode_latents`` for them (jen1_amd.encodec.EncodecHIP:
        the residual search writes the latents itself).
        ``normalizer`` (keyword-only; the reference has only an empty stub): the ``jen1_amd.normalizer.Normalizer`` the model was trained
        behind.  None: the one saved in the checkpoint's ``'normalizer'`` entry when the file has one, else no normalisation.  With one,
        the known latents are normalised right behind ``get_emb`` and the sampler's result is denormalised right in front of the decoder:
        masks, ``preserve_known``, windows and the samplers work in the normalised space, as training does."""
        if weights not in ("model", "ema"):
            raise ValueError(f"weights must be 'model' or 'ema', not {weights!r}")
        if latents not in ("codes", "fused"):
            raise ValueError(f"latents must be 'codes' or 'fused', not {latents!r}")
        if latents == "fused" and not hasattr(audio_encoder, "encode_latents"):
            raise ValueError("latents='fused' needs an audio_encoder with encode_latents (jen1_amd.encodec.EncodecHIP)")
        self.latents, self.normalizer = latents, normalizer
        self.ckpt_path, self.device, self.sample_rate, self.weights = ckpt_path, device, sample_rate, weights
        self.conditioner, self.audio_encoder = conditioner, audio_encoder
        self.cross_attn_cond_ids, self.global_cond_ids, self.input_concat_ids = cross_attn_cond_ids, global_cond_ids, input_concat_ids
        self.convert_audio = convert_audio or self._convert_audio
        self.model_config = dict(model_config or full_model_config())
        self.diffusion_config = diffusion_config or GDMConfig()
        self.vdm_config = vdm_config or VDMConfig()
        self.compute_dtype = compute_dtype
        self._model: Optional[UNetCFG1d] = None
        self.batch_size = 1

    def _convert_audio(self, wav: torch.Tensor, sr: Optional[int], target_sr: int, target_channels: int) -> torch.Tensor:
        """the default ``convert_audio``: jen1_amd.audio.convert_audio on ``self.device``; ``sr=None`` means the model's own rate.  Audio
        that needs neither resampling nor a channel conversion is returned as it is and nothing is imported or loaded."""
        sr = target_sr if sr is None else sr
        if sr == target_sr and wav.shape[-2] == target_channels:
            return wav
        from . import audio
        return audio.convert_audio(wav, sr, target_sr, target_channels, device=self.device)

    # generation.py:36-74
    def get_model_and_diffusion(self, steps: int, use_gdm: bool):
        if use_gdm:
            dc = self.diffusion_config
            betas, alphas = get_beta_schedule(dc.noise_schedule, dc.steps)
            diffusion = GaussianDiffusion(steps=dc.steps, betas=betas.to(self.device, torch.float32), alphas=alphas, objective=dc.objective,
                                          loss_type=dc.loss_type, device=self.device, cfg_dropout_proba=dc.cfg_dropout_proba,
                                          embedding_scale=dc.embedding_scale, batch_cfg=dc.batch_cfg, scale_cfg=dc.scale_cfg,
                                          sampling_timesteps=steps, use_fp16=False)
        else:                              # generation.py:54-58: the variational_diffusion block of the config
            from .vdm import VDM
            vc = self.vdm_config
            diffusion = VDM(loss_type=vc.loss_type, device=self.device, cfg_dropout_proba=vc.cfg_dropout_proba,
                            embedding_scale=vc.embedding_scale, batch_cfg=vc.batch_cfg, scale_cfg=vc.scale_cfg, use_fp16=False)
        if self._model is None:          # the reference re-creates and re-loads the model on every call; once is enough
            cfg = dict(self.model_config)
            model = UNetCFG1d(context_embedding_features=cfg.pop("context_embedding_features", None),
                              context_embedding_max_length=cfg.pop("context_embedding_max_length", None),
                              compute_dtype=self.compute_dtype, device=self.device, **cfg)
            if self.ckpt_path is not None:
                model, _, _, _ = load_checkpoint(self.ckpt_path, model, weights=self.weights)
                if self.normalizer is None:
                    self.normalizer = load_normalizer(self.ckpt_path)
            self._model = model.eval()
        return diffusion, self._model

    # ------------------------------------------------------------------ generate (generation.py:76-132)
    #
    # A request is planned in three independent pieces and only then touches the device:
    #   _task_window   which seconds are to be generated (the mask is 0 there) and whether the denoiser runs causally
    #   _known_audio   the waveform whose latents are "known": silence, the given audio, or the given prefix + placeholder
    #   _sample        latents of the known audio -> conditioning dict -> DDIM loop on the HIP path -> decoder
    def _task_window(self, task: str, seconds: float, inpainting_scope, prefix_samples: int) -> Tuple[float, float, bool]:
        """(start_s, end_s, causal): text_guided generates everything, music_inpaint the given scope, music_cont everything
        behind the given prefix with the causal network (generation.py:96-110)"""
        if task == "text_guided":
            return 0.0, float(seconds), False
        if task == "music_inpaint":
            if inpainting_scope is None or len(inpainting_scope) != 2:
                raise ValueError("music_inpaint needs inpainting_scope=(start_s, end_s)")
            return float(inpainting_scope[0]), float(inpainting_scope[1]), False
        if task == "music_cont":
            return prefix_samples / self.sample_rate, float(seconds), True
        raise ValueError(f"unknown task {task!r}")

    def _known_audio(self, task: str, init_audio: Optional[torch.Tensor], init_audio_sr: Optional[int], batch_size: int,
                     total_samples: int) -> Tuple[torch.Tensor, bool, int]:
        """([B, channels, n] waveform in the model's sample rate / channel count, whether it is only a placeholder, the number of
        samples of the given audio AFTER conversion to the model's sample rate -- generation.py:103 reads ``init_audio.size(2)``
        behind ``convert_audio``, so the continuation starts where the resampled prefix ends).
        Without ``init_audio`` the known audio is silence and the sampler starts from noise; audio without a batch axis is
        repeated over the batch; for music_cont the prefix is extended to the full length (the extension is masked out, its
        content never reaches the network)."""
        channels = self.audio_encoder.channels
        if init_audio is None:
            return torch.zeros((batch_size, channels, total_samples)), True, 0
        if init_audio.dim() == 2:
            init_audio = init_audio.unsqueeze(0).expand(batch_size, -1, -1)
        wav = self.convert_audio(init_audio, init_audio_sr, self.sample_rate, channels)
        prefix = int(wav.shape[2])
        if task == "music_cont":
            missing = total_samples - wav.shape[2]
            if missing < 0:
                raise ValueError("music_cont: init_audio is longer than the requested duration")
            # the reference appends noise * mask here (generation.py:105-107); the mask is 0 over the whole extension
            wav = torch.cat([wav, wav.new_zeros((wav.shape[0], wav.shape[1], missing))], dim=2)
        return wav, False, prefix

    @staticmethod
    def _metadata_rows(prompt, batch_size: int, conditions):
        """the conditioner's metadata rows: None without ``conditions`` (the call stays ``[{"prompt": prompt}] * B``), else one dict per
        batch row with the entries of ``conditions`` merged in"""
        if conditions is None:
            return None
        if isinstance(conditions, dict):
            conditions = [conditions] * batch_size
        conditions = list(conditions)
        if len(conditions) != batch_size or not all(isinstance(c, dict) for c in conditions):
            raise ValueError(f"conditions must be a dict or a list of batch_size = {batch_size} dicts")
        return [{"prompt": prompt, **c} for c in conditions]

    def generate(self, prompt, seed: int = -1, steps: int = 100, batch_size: int = 1, seconds: int = 30, use_gdm: bool = False,
                 task: str = "text_guided", init_audio: Optional[torch.Tensor] = None, init_audio_sr: Optional[int] = None,
                 inpainting_scope=None, sampler: Optional[str] = None, output_sr: Optional[int] = None,
                 decode: str = "whole", segment_scales: str = "unit", conditions=None,
                 window_seconds: Optional[float] = None, window_overlap: float = 0.5, ceiling_dbtp: float = -1.0,
                 lookahead_ms: float = 1.5, release_ms: float = 100.0, normalize: Optional[str] = None,
                 target_lufs=-14.0, limit: str = "clip", preserve_known: bool = False) -> torch.Tensor:
        """``normalize`` / ``target_lufs`` / ``limit`` (not in the reference): set the level of the decoder's output, which otherwise comes
        back as the codec leaves it (Encodec 48 kHz decodes every segment at unit RMS: peaks far above full scale, hard-clipped by a
        16-bit writer).  ``normalize``: a strategy of ``jen1_amd.audio.normalize_audio`` -- "loudness" (BS.1770-4 integrated loudness
        brought to ``target_lufs``), "peak", "rms" or "clip" -- applied with ``limit`` ("none", "clip", "tanh") on the device the
        decoder left its output on, at the model's rate, BEFORE the ``output_sr`` resample.  ``target_lufs="input"`` (music_inpaint /
        music_cont with ``init_audio``): each row's target is the measured loudness of its own given audio after conversion.  None
        keeps the call as it was, bit for bit.
        ``limit="truepeak"`` with ``ceiling_dbtp`` / ``lookahead_ms`` / ``release_ms`` (read by this limit alone, and like every limit only
        with ``normalize``): the gain is applied with no limit at the model's rate, and ``jen1_amd.audio.limit_true_peak`` runs LAST, behind
        the ``output_sr`` resample, on the audio at the rate the caller receives -- a ceiling promised in front of a resampler is not kept by it.
        ``window_seconds`` / ``window_overlap`` (not in the reference): long-form generation.  With ``seconds > window_seconds`` the
        piece is not handed to the denoiser as one sample of a length it was never trained on: its latents live on one canvas of L
        frames and are denoised as W overlapping windows of T frames -- T the frame count the encoder gives ``window_seconds``,
        hop = max(1, round(T * (1 - window_overlap))) -- which run as ordinary batch rows (``batch_size * W`` of them) and are merged
        on the canvas after every sampler step (``jen1_amd.windows``, ``sample_windows``).  The known audio is encoded for the whole
        length as always; ``masked_input`` and ``mask`` are built on the canvas and gathered per window row, so here the concat context
        is PER ROW -- a deviation from ``get_conditioning``'s first-element quirk, which cannot hold when windows differ.  ``prompt``
        may be one string or a list of W strings (one per window, the same for every piece) and ``conditions`` additionally a list of
        ``batch_size * W`` dicts (row ``s * W + j`` = window j of piece s).  ``preserve_known``, every ``sampler``, ``decode``,
        ``segment_scales`` and ``output_sr`` act on the canvas latents unchanged.  With ``seconds <= window_seconds`` (or None) the call
        is the call without the keywords, bit for bit.
        ``conditions`` (not in the reference, whose ``generate`` can only pass a prompt): further metadata for the conditioner --
        a dict (the same for every row) or a list of ``batch_size`` dicts -- merged into the ``{"prompt": prompt}`` rows before the
        conditioner is called (``jen1_amd.conditioners.MultiConditionerHIP``: tempo, key, seconds_start, ...); the entries named by
        ``global_cond_ids`` reach the denoiser as ``features``.  None keeps the call as it was.
        ``decode`` (not in the reference): ``"whole"`` hands all latents to ``audio_encoder.decoder`` in one piece, as generation.py:130
        does -- the latents hold the encoder's overlapping 1 s segments side by side, so 10 s come back as 1515 x 320 samples with every
        overlap played twice; ``"segments"`` undoes the encoder's layout with the codec's own decode (``audio_encoder.decode_latents``:
        per-segment decoder, linear overlap-add) and returns exactly ``seconds * sample_rate`` samples.
        ``segment_scales`` (not in the reference, nor in the ``encodec`` package; ``decode="segments"`` only): ``"unit"`` decodes every
        segment at unit RMS, which is what the reference's decoder call amounts to; ``"known"`` gives a segment that lies wholly inside the
        kept region of the known audio the scale its encoder measured, and every other segment the RMS of those scales
        (``known_segment_scales``), so kept audio comes back at its own level.
        ``preserve_known`` (not in the reference): for music_inpaint / music_cont, pin the frames the mask keeps to the latents of
        the given audio (the samplers' ``known`` / ``keep_mask``) instead of regenerating them from the conditioning alone.
        ``sampler="dpmpp2m"`` (not in the reference; ``use_gdm=True`` only): DPM-Solver++(2M) over ``steps`` network evaluations,
        ``GaussianDiffusion.dpm_sample``; None keeps the reference's samplers.
        ``output_sr`` (not in the reference): return the audio at this sample rate instead of the model's, resampled by
        ``jen1_amd.audio.resample`` (the HIP kernel of ``convert_audio``); None or the model's own rate changes nothing."""
        if output_sr is not None and int(output_sr) <= 0:
            raise ValueError(f"output_sr must be a positive sample rate, not {output_sr!r}")
        if sampler not in (None, "dpmpp2m"):
            raise ValueError(f"unknown sampler {sampler!r}: None or 'dpmpp2m'")
        if sampler is not None and not use_gdm:
            raise ValueError("sampler='dpmpp2m' needs use_gdm=True: there is no multistep solver for the variational diffusion model")
        if preserve_known and task == "text_guided":
            raise ValueError("preserve_known needs known audio: task 'music_inpaint' or 'music_cont'")
        if decode not in ("whole", "segments"):
            raise ValueError(f"unknown decode {decode!r}: 'whole' or 'segments'")
        if segment_scales not in ("unit", "known"):
            raise ValueError(f"unknown segment_scales {segment_scales!r}: 'unit' or 'known'")
        if segment_scales == "known" and decode != "segments":
            raise ValueError("segment_scales='known' needs decode='segments': the whole-latent decoder call has no per-segment scale")
        if segment_scales == "known" and task == "text_guided":
            raise ValueError("segment_scales='known' needs known audio: task 'music_inpaint' or 'music_cont'")
        if decode == "segments" and not hasattr(self.audio_encoder, "decode_latents"):
            raise ValueError("decode='segments' needs an audio_encoder with decode_latents (jen1_amd.encodec.EncodecHIP)")
        if normalize is not None:
            from . import audio
            if normalize not in audio.STRATEGIES:
                raise ValueError(f"unknown normalize {normalize!r}: None or one of {audio.STRATEGIES}")
            if limit not in audio.LIMITS:
                raise ValueError(f"unknown limit {limit!r}: one of {audio.LIMITS}")
            audio.hop_samples(self.sample_rate)
            if limit == "truepeak":
                audio.limiter_plan(self.sample_rate if output_sr is None else int(output_sr), ceiling_dbtp, lookahead_ms, release_ms)
            if isinstance(target_lufs, str):
                if target_lufs != "input":
                    raise ValueError(f"target_lufs must be a number, a tensor or 'input', not {target_lufs!r}")
                if task == "text_guided" or init_audio is None:
                    raise ValueError("target_lufs='input' needs known audio: task 'music_inpaint' or 'music_cont' with init_audio")
        windowed = self._check_windows(seconds, window_seconds, window_overlap)
        rows = None if windowed else self._metadata_rows(prompt, batch_size, conditions)
        torch.manual_seed(seed if seed != -1 else int(np.random.randint(0, 2 ** 32 - 1)))
        self.batch_size = batch_size
        diffusion, model = self.get_model_and_diffusion(steps, use_gdm)
        total = int(seconds * self.sample_rate)
        wav, placeholder, prefix = self._known_audio(task, init_audio, init_audio_sr, batch_size, total)
        start_s, end_s, causal = self._task_window(task, seconds, inpainting_scope, prefix)
        keep = self.get_mask(total, start_s, end_s, batch_size)                 # 1 = keep the known audio, 0 = generate
        out = self._sample(diffusion, model, prompt, wav, keep, causal, seed_with_audio=not placeholder, steps=steps,
                           preserve_known=preserve_known, sampler=sampler, decode=decode, segment_scales=segment_scales, length=total,
                           metadata=rows, windows=(float(window_seconds), float(window_overlap), conditions) if windowed else None)
        if normalize is not None:
            from . import audio
            on = out.device if out.device.type == "cuda" else self.device
            if isinstance(target_lufs, str):                   # "input": the level of each row's given audio, measured where the output is
                target_lufs = audio.loudness(wav[:, :, :prefix].to(on), self.sample_rate, device=on)
            out = audio.normalize_audio(out, self.sample_rate, strategy=normalize, target_lufs=target_lufs,
                                        limit="none" if limit == "truepeak" else limit, device=on)
        if output_sr is not None and int(output_sr) != self.sample_rate:
            from . import audio
            # on the device the decoder left its output on; a CPU decoder's output goes through the model's device and comes back
            out = audio.resample(out, self.sample_rate, int(output_sr), device=out.device if out.device.type == "cuda" else self.device)
        if normalize is not None and limit == "truepeak":
            out = audio.limit_true_peak(out, self.sample_rate if output_sr is None else int(output_sr), ceiling_dbtp=ceiling_dbtp,
                                        lookahead_ms=lookahead_ms, release_ms=release_ms,
                                        device=out.device if out.device.type == "cuda" else self.device)
        return out

    @staticmethod
    def _check_windows(seconds, window_seconds, window_overlap) -> bool:
        """the ``window_seconds`` / ``window_overlap`` keywords: ValueError for values that make no plan, else whether the windowed path
        is taken (a piece no longer than a window is today's call)"""
        if window_seconds is None:
            return False
        if not float(window_seconds) > 0:
            raise ValueError(f"window_seconds must be positive, not {window_seconds!r}")
        if not 0.0 <= float(window_overlap) < 1.0:
            raise ValueError(f"window_overlap must be in [0, 1), not {window_overlap!r}")
        return float(seconds) > float(window_seconds)

    def _window_rows(self, prompt, batch_size: int, W: int, conditions):
        """the conditioner's metadata for the ``batch_size * W`` window rows (row s W + j = window j of piece s): ``prompt`` one string or
        W of them, ``conditions`` None, one dict, ``batch_size`` dicts (one per piece) or ``batch_size * W`` (one per row)"""
        if isinstance(prompt, (list, tuple)):
            if len(prompt) != W:
                raise ValueError(f"prompt is a list of {len(prompt)} strings, the piece has W = {W} windows")
            prompts = list(prompt) * batch_size
        else:
            prompts = [prompt] * (batch_size * W)
        if conditions is None:
            extra = [{}] * (batch_size * W)
        elif isinstance(conditions, dict):
            extra = [conditions] * (batch_size * W)
        else:
            extra = list(conditions)
            if len(extra) == batch_size and W > 1:
                extra = [c for c in extra for _ in range(W)]
            if len(extra) != batch_size * W or not all(isinstance(c, dict) for c in extra):
                raise ValueError(f"conditions must be a dict or a list of batch_size = {batch_size} or batch_size * W = {batch_size * W} dicts")
        return [{"prompt": p, **c} for p, c in zip(prompts, extra)]

    def _sample_windows(self, diffusion, model, prompt, known, keep, causal, seed_with_audio, steps, preserve_known, sampler, n_samples,
                        window_seconds, window_overlap, conditions) -> torch.Tensor:
        """the windowed form of the sampler call of ``_sample``: canvas latents [B, 128, L] of the known audio -> WindowPlan -> per-row
        conditioning -> ``sample_windows``"""
        from .windows import WindowPlan
        B, _, Lc = known.shape
        n_win = int(window_seconds * self.sample_rate)
        frames = getattr(self.audio_encoder, "segment_frames", None)          # (EncodecHIP: encodec.segment_frame_counts)
        T = sum(frames(n_win)) if frames is not None else round(Lc * n_win / n_samples)
        T = max(1, min(int(T), Lc))
        plan = WindowPlan(Lc, T, max(1, round(T * (1.0 - window_overlap))))
        cond = self.conditioner(self._window_rows(prompt, B, plan.W, conditions), self.device)
        for k in self.global_cond_ids:
            if k not in cond:
                raise KeyError(f"global_cond_ids names {k!r}, which the conditioner did not return (it returned {sorted(cond)})")
        # the concat context per row: every window sees its own crop of the masked known audio and of the mask
        cond = get_conditioning(cond, self.cross_attn_cond_ids, self.global_cond_ids, ())
        if len(self.input_concat_ids) > 0:
            canvas = {"masked_input": known * keep, "mask": keep}
            cond["input_concat_cond"] = torch.cat([plan.gather(canvas[k].contiguous()) for k in self.input_concat_ids], dim=1)
        extra = {"sampler": sampler} if isinstance(diffusion, GaussianDiffusion) else {"step": steps}
        if seed_with_audio:              # (``init_data`` of the plain call: the given audio's latents added to the start noise)
            noise = torch.randn(tuple(known.shape), device=self.device)
            extra.update(init_noise=noise + known, known_noise=noise if preserve_known else None)
        if preserve_known:
            extra.update(known=known, keep_mask=keep)
        return diffusion.sample_windows(model, plan, B, cond, causal=causal, **extra)

    def _sample_plain(self, diffusion, model, prompt, known, keep, causal, seed_with_audio, steps, preserve_known, sampler, metadata):
        """the sampler call of ``_sample`` for a piece that is one sample of the denoiser"""
        B = known.shape[0]
        cond = self.conditioner([{"prompt": prompt}] * B if metadata is None else metadata, self.device)
        for k in self.global_cond_ids:
            if k not in cond:
                raise KeyError(f"global_cond_ids names {k!r}, which the conditioner did not return (it returned {sorted(cond)})")
        cond["masked_input"] = known * keep
        cond["mask"] = keep
        cond = self.get_conditioning(cond)
        extra = {} if isinstance(diffusion, GaussianDiffusion) else {"step": steps}       # VDM.sample takes the step count itself (vdm.py:77)
        if preserve_known:               # (the concat context is the FIRST sample's, get_conditioning; the blend is per sample)
            extra.update(known=known, keep_mask=keep)
        if sampler is not None:
            extra["sampler"] = sampler
        return diffusion.sample(model, tuple(known.shape), cond, causal=causal, init_data=known if seed_with_audio else None, **extra)

    @torch.no_grad()
    def _sample(self, diffusion, model, prompt, wav: torch.Tensor, keep: torch.Tensor, causal: bool, seed_with_audio: bool,
                steps: int = 100, preserve_known: bool = False, sampler: Optional[str] = None, decode: str = "whole",
                segment_scales: str = "unit", length: Optional[int] = None, metadata=None, windows=None) -> torch.Tensor:
        B = wav.shape[0]
        keep_samples = keep
        if decode == "segments":
            known, seg_frames, enc_scales = self.get_emb_segments(wav.to(self.device))
            known = known.to(self.device)
        else:
            known = self.get_emb(wav.to(self.device)).to(self.device)           # [B, 128, T']
        if self.normalizer is not None:    # from here to the decoder everything lives in the normalised space, as in training
            known = self.normalizer.normalize(known.to(torch.float32))
        keep = torch.nn.functional.interpolate(keep.to(self.device), size=known.shape[2])
        if windows is not None:
            z = self._sample_windows(diffusion, model, prompt, known, keep, causal, seed_with_audio, steps, preserve_known, sampler,
                                     wav.shape[-1], *windows)
        else:
            z = self._sample_plain(diffusion, model, prompt, known, keep, causal, seed_with_audio, steps, preserve_known, sampler, metadata)
        if self.normalizer is not None:
            z = self.normalizer.denormalize(z.to(torch.float32))
        # the reference hands the latents to its CPU decoder (generation.py:129-130); a decoder that lives on a device says so
        # (EncodecHIP.decoder_device) and gets them where they are
        if decode == "segments":
            scales = None
            if segment_scales == "known":
                if enc_scales is None:
                    raise ValueError("segment_scales='known': the audio_encoder's encode returned no scales (normalize=False)")
                ae = self.audio_encoder
                offs = range(0, wav.shape[-1], ae.segment_stride)
                scales = known_segment_scales(enc_scales, keep_samples, [(o, min(ae.segment_length, wav.shape[-1] - o)) for o in offs])
            return self.audio_encoder.decode_latents(z.to(getattr(self.audio_encoder, "decoder_device", "cpu")), seg_frames, scales=scales,
                                                     length=wav.shape[-1] if length is None else min(length, wav.shape[-1]))
        return self.audio_encoder.decoder(z.to(getattr(self.audio_encoder, "decoder_device", "cpu")))

    # generation.py:134-150
    def get_mask(self, sample_size: int, start: float, end: float, batch_size: int) -> torch.Tensor:
        return get_mask(sample_size, start, end, batch_size, self.sample_rate)

    def get_emb(self, audio: torch.Tensor) -> torch.Tensor:
        """waveform -> continuous latents [B, 128, T']: the codes of every encoded segment side by side in time, summed
        codebook vectors (generation.py:145-150)"""
        if self.latents == "fused":
            return self.audio_encoder.encode_latents(audio)[0]
        per_segment = [codes for codes, _scale in self.audio_encoder.encode(audio)]          # each [B, n_q, T_seg]
        return self.audio_encoder.quantizer.decode(torch.cat(per_segment, dim=-1).permute(1, 0, 2))

    def get_emb_segments(self, audio: torch.Tensor):
        """``get_emb`` together with the layout it came from: (latents [B, 128, T'], the frame count of every segment, the encoder's
        per-segment scales [B, S] or None) -- what ``decode_latents`` needs to undo the segmentation"""
        if self.latents == "fused":
            return self.audio_encoder.encode_latents(audio)
        frames = self.audio_encoder.encode(audio)
        emb = self.audio_encoder.quantizer.decode(torch.cat([codes for codes, _ in frames], dim=-1).permute(1, 0, 2))
        scales = None
        if all(s is not None for _, s in frames):
            scales = torch.cat([s.reshape(-1, 1).to(torch.float32) for _, s in frames], dim=1)
        return emb, [int(codes.shape[-1]) for codes, _ in frames], scales

    @torch.no_grad()
    def codec_report(self, wav: torch.Tensor, sr: Optional[int] = None) -> dict:
        """What the codec alone costs on ``wav`` (``[C, n]`` or ``[B, C, n]`` at rate ``sr``; None: the model's own): the audio is converted as
        ``generate`` converts ``init_audio``, encoded with ``encode_latents`` and decoded with ``decode_latents`` (segment by segment, to the
        exact length), and the result is ``jen1_amd.spectral.audio_report(reconstruction, converted input, sample_rate)`` -- the floor
        under every generation metric.  Not in the reference."""
        ae = self.audio_encoder
        if not hasattr(ae, "encode_latents"):
            raise ValueError("codec_report needs an audio_encoder with encode_latents (jen1_amd.encodec.EncodecHIP)")
        if not hasattr(ae, "decode_latents"):
            raise ValueError("codec_report needs an audio_encoder with decode_latents (jen1_amd.encodec.EncodecHIP)")
        from . import spectral
        if wav.dim() == 2:
            wav = wav.unsqueeze(0)
        x = self.convert_audio(wav, sr, self.sample_rate, ae.channels).to(self.device)
        z, seg_frames, scales = ae.encode_latents(x)
        y = ae.decode_latents(z.to(getattr(ae, "decoder_device", "cpu")), seg_frames, scales=scales, length=x.shape[-1])
        return spectral.audio_report(y.to(self.device), x, self.sample_rate, device=self.device)

    def control_report(self, wav: torch.Tensor, sr: Optional[int] = None, conditions=None) -> dict:
        """How ``wav`` (``[C, n]`` or ``[B, C, n]`` at rate ``sr``; None: the model's own) follows the global controls it was asked for: the
        audio is converted as ``codec_report`` converts it and the result is ``jen1_amd.analysis.control_report`` -- the measured tempo and
        key of every row, and against the ``"tempo"`` / ``"key"`` entries of ``conditions`` (the dict ``generate`` took, or one per row)
        the verdicts ``tempo_match``, ``tempo_match_octave``, ``key_match`` and ``key_related``.  Not in the reference."""
        from . import analysis
        if wav.dim() == 2:
            wav = wav.unsqueeze(0)
        x = self.convert_audio(wav, sr, self.sample_rate, self.audio_encoder.channels).to(self.device)
        rows = [conditions or {}] * int(x.shape[0]) if not isinstance(conditions, (list, tuple)) else list(conditions)
        if len(rows) != int(x.shape[0]):
            raise ValueError(f"control_report: {len(rows)} condition dicts for {int(x.shape[0])} rows")
        target = lambda name: None if all(name not in c for c in rows) else [c.get(name) for c in rows]
        tempo, key = target("tempo"), target("key")
        if any(v is None for t in (tempo, key) if t is not None for v in t):
            raise ValueError("control_report: a control is given for some rows only")
        return analysis.control_report(x, self.sample_rate, tempo=tempo, key=key, device=self.device)

    # generation.py:152-192
    def get_conditioning(self, cond):
        """as written in the reference: input-concat entries are read as ``cond[key][0]`` -- the FIRST batch element --
        and expanded over the batch (generation.py:173-180)"""
        return get_conditioning(cond, self.cross_attn_cond_ids, self.global_cond_ids, self.input_concat_ids, batch_size=self.batch_size)


# generation.py:194-213
def save_audio_tensor(audio_tensor: torch.Tensor, file_path: str, sample_rate: int = 48000, normalize: Optional[str] = None,
                      target_lufs=-14.0, limit: str = "clip", ceiling_dbtp: float = -1.0, lookahead_ms: float = 1.5,
                      release_ms: float = 100.0) -> None:
    """saves audio ``[C, N]`` (or ``[1, C, N]``: the batch axis is dropped) as a 16-bit PCM ``.wav`` file (``jen1_amd.wav.save`` in the place
    of ``torchaudio.save``).  ``normalize`` / ``target_lufs`` / ``limit`` (not in the reference): ``jen1_amd.audio.normalize_audio`` at
    ``sample_rate`` in front of the writer, on the tensor's GPU or the current one; None writes the samples as they are.  ``ceiling_dbtp`` /
    ``lookahead_ms`` / ``release_ms``: the keywords of ``limit="truepeak"``."""
    from . import wav
    audio_tensor = audio_tensor.detach()
    if audio_tensor.ndim == 3:
        audio_tensor = audio_tensor.squeeze(0)
    if normalize is not None:
        from . import audio
        audio_tensor = audio.normalize_audio(audio_tensor.to(torch.float32), sample_rate, strategy=normalize, target_lufs=target_lufs, limit=limit,
                                             device=audio_tensor.device if audio_tensor.device.type == "cuda" else "cuda",
                                             ceiling_dbtp=ceiling_dbtp, lookahead_ms=lookahead_ms, release_ms=release_ms)
    wav.save(file_path, audio_tensor.to("cpu", torch.float32), sample_rate)
