"""Denoise loop of ``LTXVideoPipeline.__call__`` (text-/image-/video-to-video) with everything on device.

Mirrors ltx_video/pipelines/pipeline_ltx_video.py:919-1307 for the inputs the hot path sees:
pre-computed prompt embeddings (the T5 encoder is outside this path), optional conditioning
items (``ConditioningItem`` :203-219, ``prepare_conditioning`` :1344-1548), ``joint_pass=True``.
Per step (pipeline_ltx_video.py:1104-1256):

    latent_model_input = cat([latents] * num_conds)            (:1115)
    noise_pred = transformer(...)                               (:1160-1179)   <- libltxmi
    CFG-star / STG / std-rescale + scheduler.step (Euler)       (:1183-1241)   <- one fused
                                                                   ltxmi_guidance_step_bf16

The reference's per-step host work (``skip_layer_mask.min()`` per block, ``.item()`` calls,
Python float timesteps) is replaced by host-side schedule scalars computed once (``_StepPlan``); no
host<->device synchronisation happens inside the loop.
"""
import copy
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from . import ops
from .attention import SkipLayerStrategy
from .autoencoder import randn_rows, vae_decode, vae_encode
from .patchifier import SymmetricPatchifier, latent_to_pixel_coords_from_factors


@dataclass
class ConditioningItem:
    """pipeline_ltx_video.py:203-219: a frame (f = 1) or frame sequence (f = 8k+1) to condition on."""
    media_item: torch.Tensor                 # (b, 3, f, h, w) in [-1, 1]
    media_frame_number: int
    conditioning_strength: float
    media_x: Optional[int] = None
    media_y: Optional[int] = None


def _refuse(rows):
    """Walk ``(refused, exception type, message)`` rows in order and raise the first one that applies."""
    for refused, error, message in rows:
        if refused:
            raise error("ltxmi.LTXVideoPipeline: " + message)


def _shape(x):
    return None if x is None else tuple(x.shape)


def _randn(shape, generator, device, dtype):
    """Every draw of the pipeline: ``randn_rows`` (a generator list gives video j what its single call draws)."""
    return randn_rows(shape, generator, device, dtype, randn=torch.randn)


def _resize_frames(video, height, width):
    """(b, c, f, h, w) -> (b, c, f, height, width): torch's bilinear resize, frame by frame (host-side pre- / post-processing)."""
    frames = video.transpose(1, 2).flatten(0, 1)
    frames = torch.nn.functional.interpolate(frames, size=(height, width), mode="bilinear", align_corners=False)
    return frames.unflatten(0, (-1, video.shape[2])).transpose(1, 2)


def retrieve_timesteps(scheduler, num_inference_steps=None, device=None, timesteps=None, max_timestep=1.0,
                       skip_initial_inference_steps=0, skip_final_inference_steps=0, **kwargs):
    """pipeline_ltx_video.py:125-198: the scheduler's (or the given) schedule, minus skipped head/tail
    steps, truncated to ``max_timestep``; the scheduler is re-set to exactly the returned list."""
    asked = {"num_inference_steps": num_inference_steps} if timesteps is None else {"timesteps": timesteps}
    scheduler.set_timesteps(device=device, **asked, **kwargs)
    schedule = list(scheduler.host_timesteps)
    head, tail = skip_initial_inference_steps, skip_final_inference_steps
    if head < 0 or tail < 0 or head + tail >= len(schedule):
        raise ValueError(f"ltxmi.retrieve_timesteps: skip_initial_inference_steps={head} and skip_final_inference_steps="
                         f"{tail} must be >= 0 and leave at least one of the {len(schedule)} steps")
    schedule = schedule[head: len(schedule) - tail]
    if max_timestep < 1.0:
        if max_timestep < min(schedule):
            raise ValueError(f"ltxmi.retrieve_timesteps: max_timestep={max_timestep} lies below the whole schedule "
                             f"(its last step is {min(schedule)})")
        schedule = [t for t in schedule if t <= max_timestep]
    scheduler.set_timesteps(timesteps=schedule, device=device, **kwargs)
    return list(scheduler.host_timesteps), len(schedule)


class LTXVideoPipeline:
    """Same constructor keywords, attributes and ``__call__`` signature as the reference's pipeline
    (pipeline_ltx_video.py:222-304, 762-807), so ``ltxv.py:420-445`` calls through unchanged.  The text encoder
    is outside this path: ``tokenizer`` / ``text_encoder`` are whatever the caller has (the HF T5 objects the
    reference loads, ``ltxv.py:186-192``) and are only touched by ``encode_prompt``; the prompt enhancer models
    are accepted and never used (``enhance_prompt=True`` raises)."""

    def __init__(self, tokenizer=None, text_encoder=None, vae=None, transformer=None, scheduler=None, patchifier=None,
                 prompt_enhancer_image_caption_model=None, prompt_enhancer_image_caption_processor=None,
                 prompt_enhancer_llm_model=None, prompt_enhancer_llm_tokenizer=None,
                 allowed_inference_steps: Optional[List[float]] = None):
        self.tokenizer, self.text_encoder = tokenizer, text_encoder
        self.vae, self.transformer, self.scheduler = vae, transformer, scheduler
        self.patchifier = patchifier or SymmetricPatchifier(patch_size=1)
        self.prompt_enhancer_image_caption_model = prompt_enhancer_image_caption_model
        self.prompt_enhancer_image_caption_processor = prompt_enhancer_image_caption_processor
        self.prompt_enhancer_llm_model = prompt_enhancer_llm_model
        self.prompt_enhancer_llm_tokenizer = prompt_enhancer_llm_tokenizer
        self.allowed_inference_steps = allowed_inference_steps
        self.video_scale_factor, self.vae_scale_factor = 8, 32         # get_vae_size_scale_factor of the LTX VAEs (:300-302)
        self._interrupt = False

    @property
    def _execution_device(self):
        return self.transformer.device

    # ---- prompt side (pipeline_ltx_video.py:315-485, 513-606): host checks and the hand-over to the caller's T5 ----
    def check_inputs(self, prompt, height, width, negative_prompt, prompt_embeds=None, negative_prompt_embeds=None,
                     prompt_attention_mask=None, negative_prompt_attention_mask=None, enhance_prompt=False):
        """Refuse argument sets the call cannot honour; the first row that applies is the one reported."""
        text, embeds, negative_embeds = prompt is not None, prompt_embeds is not None, negative_prompt_embeds is not None
        pair = embeds and negative_embeds
        _refuse([
            (height % 8 or width % 8, ValueError, f"height and width must be multiples of 8, got {height} x {width}"),
            (text and embeds, ValueError, "prompt and prompt_embeds are alternatives, pass one of them"),
            (not text and not embeds, ValueError, "one of prompt / prompt_embeds is required"),
            (text and not isinstance(prompt, (str, list)), ValueError,
             f"prompt is a str or a list of str, not {type(prompt).__name__}"),
            (text and negative_embeds, ValueError, "negative_prompt_embeds goes with prompt_embeds, not with a text prompt"),
            (negative_prompt is not None and negative_embeds, ValueError,
             "negative_prompt and negative_prompt_embeds are alternatives, pass one of them"),
            (embeds and prompt_attention_mask is None, ValueError, "prompt_embeds comes with its prompt_attention_mask"),
            (negative_embeds and negative_prompt_attention_mask is None, ValueError,
             "negative_prompt_embeds comes with its negative_prompt_attention_mask"),
            (pair and _shape(prompt_embeds) != _shape(negative_prompt_embeds), ValueError,
             f"prompt_embeds {_shape(prompt_embeds)} and negative_prompt_embeds {_shape(negative_prompt_embeds)} differ in shape"),
            (pair and _shape(prompt_attention_mask) != _shape(negative_prompt_attention_mask), ValueError,
             f"prompt_attention_mask {_shape(prompt_attention_mask)} and negative_prompt_attention_mask "
             f"{_shape(negative_prompt_attention_mask)} differ in shape"),
            (enhance_prompt, NotImplementedError, "enhance_prompt (Florence / LLM prompt rewriting) is outside this path"),
        ])

    def _encode_texts(self, texts, num_tokens, device, dtype):
        """``texts`` (stripped; padded / truncated to ``num_tokens``) through the caller's tokenizer and text encoder:
        (embeds (n, num_tokens, d) in ``dtype``, attention mask (n, num_tokens)), both on ``device``."""
        if self.text_encoder is None or self.tokenizer is None:
            raise RuntimeError("ltxmi.LTXVideoPipeline.encode_prompt: text prompts (the negative one included) need the "
                               "caller's T5 (`tokenizer=` and `text_encoder=` at construction; `ltxmi.T5EncoderModel` / "
                               "`ltxmi.loading.load_t5_encoder` is this library's encoder, the tokenizer is the caller's); "
                               "alternatively pass the embeddings and their attention masks")
        t5_device = next(self.text_encoder.parameters()).device
        tokens = self.tokenizer([text.strip() for text in texts], padding="max_length", max_length=num_tokens,
                                truncation=True, add_special_tokens=True, return_tensors="pt")
        mask = tokens.attention_mask.to(t5_device)
        embeds = self.text_encoder(tokens.input_ids.to(t5_device), attention_mask=mask)[0]
        return embeds.to(device=device, dtype=dtype), mask.to(device)

    @staticmethod
    def _per_image(embeds, mask, num_images):
        """Every row ``num_images`` times, prompt-major: (p0, p0, p1, p1, ...)."""
        return embeds.repeat_interleave(num_images, dim=0), mask.repeat_interleave(num_images, dim=0)

    def encode_prompt(self, prompt, do_classifier_free_guidance: bool = True, negative_prompt: str = "",
                      num_images_per_prompt: int = 1, device=None, prompt_embeds=None, negative_prompt_embeds=None,
                      prompt_attention_mask=None, negative_prompt_attention_mask=None,
                      text_encoder_max_tokens: int = 256, **kwargs):
        """:315-485.  The positive and (under guidance) the negative (embeds, mask) pair, each either encoded by the
        caller's text encoder or taken as given, cast to the text encoder's (else the transformer's) dtype and repeated
        per image.  The negative text is encoded once per prompt, at the positive pair's token length.  The T5 itself
        is not part of this library: text without ``text_encoder`` / ``tokenizer`` is an explicit error."""
        device = self._execution_device if device is None else device
        owner = self.text_encoder if self.text_encoder is not None else self.transformer
        dtype = None if owner is None else owner.dtype

        def pair(texts, embeds, mask, num_tokens, copies=1):
            if embeds is not None:
                return embeds.to(device=device, dtype=dtype), mask
            texts = [texts] if isinstance(texts, str) else list(texts)
            return self._encode_texts(texts * copies, num_tokens, device, dtype)

        positive = pair(prompt, prompt_embeds, prompt_attention_mask, text_encoder_max_tokens)
        if not do_classifier_free_guidance:
            return (*self._per_image(*positive, num_images_per_prompt), None, None)
        num_prompts, num_tokens = positive[0].shape[:2]
        negative = pair(negative_prompt, negative_prompt_embeds, negative_prompt_attention_mask, num_tokens, copies=num_prompts)
        return (*self._per_image(*positive, num_images_per_prompt), *self._per_image(*negative, num_images_per_prompt))

    @staticmethod
    def postprocess(image, output_type):
        """``self.image_processor.postprocess`` (:1299; diffusers' VaeImageProcessor, restated: PARITY UNPINNED like
        the other diffusers leaves): "pt" = (x / 2 + 0.5).clamp(0, 1), which is what ``ltxv.py:462`` undoes.  The
        numpy / PIL forms of that class do not take 5-D video tensors in the reference either."""
        if output_type == "latent":
            return image
        if output_type == "pt":
            return (image / 2 + 0.5).clamp(0, 1)
        raise ValueError(f"ltxmi.LTXVideoPipeline: output_type {output_type!r} is not available for video tensors "
                         "(use 'pt' or 'latent')")

    def prepare_latents(self, latents, media_items, timestep, latent_shape, dtype, device, generator,
                        vae_per_channel_normalize: bool = True):
        """pipeline_ltx_video.py:632-710: (b, c, f, h, w) latents = pure noise, or the given latents / the encoded
        ``media_items`` noised to ``timestep``.  The noise is drawn in PATCHIFIED order (b, f*h*w, c) (:696-699)."""
        batch, channels, frames, rows, cols = latent_shape
        if isinstance(generator, (list, tuple)) and len(generator) != batch:
            raise ValueError(f"ltxmi.LTXVideoPipeline: {len(generator)} generators for a batch of {batch}")
        assert latents is None or media_items is None, "ltxmi.LTXVideoPipeline: latents and media_items are alternatives"
        assert (latents is None and media_items is None) or timestep < 1.0, \
            "ltxmi.LTXVideoPipeline: at timestep 1 the given latents / media_items would be all noise (pass strength < 1)"
        start = latents
        if media_items is not None:
            if media_items.shape[0] not in (1, batch):
                raise ValueError(f"ltxmi.LTXVideoPipeline: media_items holds {media_items.shape[0]} videos for a batch of "
                                 f"{batch} (one per video, or one shared by all)")
            start = vae_encode(media_items.to(dtype=self.vae.dtype, device=self.vae.device), self.vae,
                               vae_per_channel_normalize=vae_per_channel_normalize)
            start = start.expand(batch, *start.shape[1:])
        if start is not None:
            assert tuple(start.shape) == tuple(latent_shape), \
                f"ltxmi.LTXVideoPipeline: latents {tuple(start.shape)} where the call needs {tuple(latent_shape)}"
            start = start.to(device=device, dtype=dtype)
        noise = _randn((batch, frames * rows * cols, channels), generator, device, dtype)
        noise = self.patchifier.unpatchify(noise, rows, cols, channels) * self.scheduler.init_noise_sigma
        return noise if start is None else timestep * noise + (1 - timestep) * start

    # ---- conditioning (pipeline_ltx_video.py:1344-1690) ---------------------------------------
    # Setup-time token assembly: slicing / lerp on small latent tensors, once per call (not per step);
    # the encoder it feeds from and everything inside the loop run on libltxmi kernels.
    @staticmethod
    def resize_tensor(media_items, height, width):                                       # :748-760
        """Host pre-processing, only taken when the media is not at the target size."""
        if tuple(media_items.shape[-2:]) == (height, width):
            return media_items
        return _resize_frames(media_items, height, width)

    @staticmethod
    def _resize_conditioning_item(item, height, width):                                  # :1550-1563
        if item.media_x or item.media_y:
            raise ValueError("ltxmi.LTXVideoPipeline: a conditioning item placed by media_x / media_y is not resized; "
                             "give its media_item at the size it should have in the frame")
        resized = copy.copy(item)
        resized.media_item = LTXVideoPipeline.resize_tensor(item.media_item, height, width)
        return resized

    def _get_latent_spatial_position(self, latents, item, height, width, strip_latent_border):   # :1566-1611
        """Where a (possibly smaller) item sits in the frame: (its latents, latent column, latent row).  Centred unless
        ``media_x`` / ``media_y`` say otherwise."""
        cell = self.vae_scale_factor
        h, w = item.media_item.shape[-2:]
        assert h <= height and w <= width, f"a {w}x{h} conditioning item does not fit a {width}x{height} frame"
        assert h % cell == 0 and w % cell == 0, f"a conditioning item's size is a multiple of {cell}, got {w}x{h}"
        left = (width - w) // 2 if item.media_x is None else item.media_x
        top = (height - h) // 2 if item.media_y is None else item.media_y
        assert left + w <= width and top + h <= height, \
            f"a {w}x{h} conditioning item at ({left}, {top}) sticks out of the {width}x{height} frame"
        if strip_latent_border:
            # one latent row / column is dropped on every side of the item that does not touch the frame's border
            # (pipeline_ltx_video.py:1598-1611); a cut on the left / top moves the item's origin by one latent
            cut_l, cut_t = int(left > 0), int(top > 0)
            cut_r, cut_b = int(left + w < width), int(top + h < height)
            hl, wl = latents.shape[-2], latents.shape[-1]
            latents = latents[..., cut_t:hl - cut_b, cut_l:wl - cut_r]
            left += cut_l * cell
            top += cut_t * cell
        return latents, left // cell, top // cell

    @staticmethod
    def _handle_non_first_conditioning_sequence(init_latents, init_conditioning_mask, latents, media_frame_number,
                                                strength, num_prefix_latent_frames=2, prefix_latents_mode="concat",
                                                prefix_soft_conditioning_strength=0.15):           # :1614-1690
        """A frame sequence that starts inside the video (pixel frame ``media_frame_number`` > 0).  Its latent frames past
        the first ``num_prefix_latent_frames`` are blended into the grid where they belong.  The prefix is handed back to
        become extra tokens ("concat"), or blended in too -- all but its first frame, at no more than
        ``prefix_soft_conditioning_strength`` -- ("soft"), or left out ("drop").  Writes ``init_latents`` and
        ``init_conditioning_mask`` in place; returns them and the kept prefix (or None)."""
        if prefix_latents_mode not in ("concat", "soft", "drop"):
            raise ValueError(f"ltxmi.LTXVideoPipeline: prefix_latents_mode is 'concat', 'soft' or 'drop', not {prefix_latents_mode!r}")
        num_frames, num_prefix = latents.shape[2], num_prefix_latent_frames
        assert num_frames >= num_prefix, "the sequence is shorter than its prefix"
        assert media_frame_number % 8 == 0, "a sequence starts on a latent frame (every 8th pixel frame)"
        first = media_frame_number // 8                                # the grid's latent frame under the sequence's first

        def blend(begin, end, weight):
            """The sequence's latent frames [begin, end) into the grid frames under them, and the mask marked."""
            under = slice(first + begin, first + end)
            init_latents[:, :, under] = torch.lerp(init_latents[:, :, under], latents[:, :, begin:end], weight)
            init_conditioning_mask[:, under] = weight

        blend(num_prefix, num_frames, strength)                        # the body
        if prefix_latents_mode == "soft":
            blend(1, num_prefix, min(prefix_soft_conditioning_strength, strength))
        prefix = latents[:, :, :num_prefix] if prefix_latents_mode == "concat" else None
        return init_latents, init_conditioning_mask, prefix

    def _pixel_coords(self, latent_coords, causal_fix=True):
        return latent_to_pixel_coords_from_factors(
            latent_coords, (self.video_scale_factor, self.vae_scale_factor, self.vae_scale_factor), causal_fix=causal_fix)

    def prepare_conditioning(self, conditioning_items, init_latents, num_frames, height, width,
                             vae_per_channel_normalize=False, generator=None, sample_posterior=True):
        """:1344-1548.  init_latents (b, c, f_l, h_l, w_l) -> (latents (b, N, c), pixel_coords (b, 3, N),
        conditioning_mask (b, N) fp32 or None, number of extra conditioning tokens in front).  A media item holds one
        clip per video of the call or one shared by all (encoded once); every draw goes through ``_randn``."""
        batch = init_latents.shape[0]
        extra_latents, extra_coords, extra_mask = [], [], []
        causal_fix = bool(getattr(self.transformer.config, "causal_temporal_positioning", True))
        init_mask = torch.zeros_like(init_latents[:, 0], dtype=torch.float32) if conditioning_items else None
        for item in conditioning_items or ():
            item = self._resize_conditioning_item(item, height, width)
            media, frame_no, strength = item.media_item, item.media_frame_number, item.conditioning_strength
            assert media.ndim == 5, "a conditioning item is (b, 3, f, h, w)"
            n_frames, (h, w) = media.shape[2], media.shape[-2:]
            assert (h, w) == (height, width) or frame_no == 0, \
                f"only an item at frame 0 may be smaller than the frame: {w}x{h} in {width}x{height} at frame {frame_no}"
            assert n_frames % 8 == 1, f"a conditioning item has 8k + 1 frames, got {n_frames}"
            assert 0 <= frame_no <= num_frames - n_frames, \
                f"frames {frame_no}..{frame_no + n_frames - 1} of a conditioning item lie outside the {num_frames}-frame video"
            if media.shape[0] not in (1, batch):
                raise ValueError(f"ltxmi.LTXVideoPipeline: a conditioning item holds {media.shape[0]} clips for a batch of "
                                 f"{batch} (one per video, or one shared by all)")
            lat = vae_encode(media.to(dtype=self.vae.dtype, device=self.vae.device), self.vae,
                             vae_per_channel_normalize=vae_per_channel_normalize, generator=generator,
                             sample_posterior=sample_posterior, num_samples=batch).to(dtype=init_latents.dtype)
            lat = lat.expand(batch, *lat.shape[1:])
            if frame_no == 0:                                          # written into the grid, at its place in the frame
                lat, x, y = self._get_latent_spatial_position(lat, item, height, width, strip_latent_border=True)
                f, y1, x1 = lat.shape[2], y + lat.shape[3], x + lat.shape[4]
                init_latents[:, :, :f, y:y1, x:x1] = torch.lerp(init_latents[:, :, :f, y:y1, x:x1], lat, strength)
                init_mask[:, :f, y:y1, x:x1] = strength
                continue
            if n_frames > 1:
                init_latents, init_mask, lat = self._handle_non_first_conditioning_sequence(
                    init_latents, init_mask, lat, frame_no, strength)
            if lat is not None:                                        # extra tokens in front, at the item's frames
                noise = _randn(lat.shape, generator, lat.device, lat.dtype)
                tokens, coords = self.patchifier.patchify(torch.lerp(noise, lat, strength))
                coords = self._pixel_coords(coords, causal_fix)
                coords[:, 0] += frame_no
                extra_latents.append(tokens)
                extra_coords.append(coords)
                extra_mask.append(torch.full(tokens.shape[:2], strength, dtype=torch.float32, device=init_latents.device))
        latents, coords = self.patchifier.patchify(init_latents)
        pixel_coords = self._pixel_coords(coords, causal_fix)
        if init_mask is None:
            return latents, pixel_coords, None, 0
        mask = self.patchifier.patchify(init_mask.unsqueeze(1))[0].squeeze(-1)
        if extra_latents:
            latents = torch.cat([*extra_latents, latents], dim=1)
            pixel_coords = torch.cat([*extra_coords, pixel_coords], dim=2)
            mask = torch.cat([*extra_mask, mask], dim=1)
        return latents, pixel_coords, mask, sum(x.shape[1] for x in extra_latents)

    retrieve_timesteps = staticmethod(retrieve_timesteps)        # (a module-level function in the reference, :125)

    @staticmethod
    def _guidance_tables(timesteps, guidance_scale, stg_scale, rescaling_scale, skip_block_list, guidance_timesteps):
        """:959-1013: per-step guidance / STG / rescale / skip-block tables (lists are indexed through
        ``guidance_timesteps``; scalars are broadcast)."""
        n = len(timesteps)
        mapping = None
        if guidance_timesteps:
            mapping = []
            for t in timesteps:
                idx = [i for i, v in enumerate(guidance_timesteps) if v <= t]
                mapping.append(idx[0] if len(idx) > 0 else len(guidance_timesteps) - 1)

        def table(v):
            if not isinstance(v, list):
                return [v] * n
            if mapping is None:
                raise ValueError("list-valued guidance parameters need `guidance_timesteps`")
            return [v[mapping[i]] for i in range(n)]

        gs = [x if x > 1.0 else 0.0 for x in table(guidance_scale)]
        stg, rs = table(stg_scale), table(rescaling_scale)
        if skip_block_list is not None:
            if len(skip_block_list) == 0 or not isinstance(skip_block_list[0], list):
                skip_block_list = [skip_block_list] * n
            else:
                skip_block_list = [skip_block_list[mapping[i]] for i in range(n)]
        return gs, stg, rs, skip_block_list

    @staticmethod
    def _refuse_outside_this_path(prompt, prompt_embeds, is_video, offload_to_cpu):
        """What the reference's ``__call__`` takes and this one does not."""
        _refuse([(refused, NotImplementedError, message) for refused, message in [
            (prompt is not None or prompt_embeds is None,
             "__call__ takes prompt_embeds / prompt_attention_mask (as the reference's loop does, :1029-1051); string "
             "prompts go through encode_prompt / LTXMultiScalePipeline with the caller's T5"),
            (not is_video, "is_video=False (single images, video_scale_factor 1) is outside this path"),
            (offload_to_cpu, "offload_to_cpu is not on this path (everything is resident in HBM)"),
        ]])

    def _initial_latents(self, latents, media_items, timestep, latent_shape, dtype, device, generator,
                         vae_per_channel_normalize):
        """The (b, c, f, h, w) grid the loop starts from (:1056-1065), in fp32 or bf16."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("ltxmi.LTXVideoPipeline: latents are kept in fp32 or bf16 (prompt_embeds' dtype by default)")
        if latents is not None and latents.dim() == 3:                                   # extension: given patchified noise
            batch, channels, frames, rows, cols = latent_shape
            assert tuple(latents.shape) == (batch, frames * rows * cols, channels), \
                f"ltxmi.LTXVideoPipeline: latents {tuple(latents.shape)} where the call needs {(batch, frames * rows * cols, channels)}"
            return self.patchifier.unpatchify(latents.to(device=device, dtype=dtype), rows, cols, channels)
        return self.prepare_latents(latents=latents, media_items=media_items, timestep=timestep, latent_shape=latent_shape,
                                    dtype=dtype, device=device, generator=generator,
                                    vae_per_channel_normalize=vae_per_channel_normalize)

    @staticmethod
    def _stochastic_step_(noise_pred, latents, t, dt, guidance, cond_mask, one_minus_mask):
        """rf.py:368-373 behind the same guidance: x0 = x - t v by the fused kernel with dt = t on a copy (tokens the mask
        holds back stay as they are), then the re-noising to t - dt; the draw comes from the global RNG, as the
        reference's torch.randn_like does (one draw for the whole batch: no per-video reproducibility is claimed).
        ``guidance`` = ops.guidance_step_'s arguments after ``dt``."""
        x0 = latents.clone()
        step_ = ops.guidance_step_ if latents.shape[0] == 1 else ops.guidance_step_batched_
        step_(noise_pred, x0, t, *guidance, cond_mask=cond_mask, t=t)
        t_next = t - dt
        renoised = (1 - t_next) * x0 + t_next * torch.randn_like(latents)
        if cond_mask is None:
            latents.copy_(renoised)
        else:
            latents.copy_(torch.where((t - 1e-6 < one_minus_mask).unsqueeze(-1), renoised, latents))

    def _decode(self, latents, output_type, is_video, vae_per_channel_normalize, decode_timestep, decode_noise_scale):
        """(b, c, f, h, w) latents -> what ``output_type`` asks for (:1270-1299).  A timestep-conditioned decoder gets the
        latents mixed with fresh noise (global RNG) at ``decode_noise_scale`` (default: ``decode_timestep``), per sample."""
        if output_type == "latent":
            return latents
        timestep = None
        if self.vae.decoder.timestep_conditioning:
            def per_sample(value):
                return torch.tensor(value if isinstance(value, list) else [value] * latents.shape[0]).to(latents.device)
            timestep = per_sample(decode_timestep)
            scale = per_sample(decode_timestep if decode_noise_scale is None else decode_noise_scale)[:, None, None, None, None]
            latents = latents * (1 - scale) + torch.randn_like(latents) * scale
        image = vae_decode(latents.to(self.vae.dtype), self.vae, is_video,
                           vae_per_channel_normalize=vae_per_channel_normalize, timestep=timestep)
        return self.postprocess(image, output_type)

    @torch.no_grad()
    def __call__(
        self,
        height: int,
        width: int,
        num_frames: int,
        frame_rate: float,
        prompt: Union[str, List[str]] = None,
        negative_prompt: str = None,
        num_inference_steps: int = 20,
        timesteps: List[int] = None,
        guidance_scale: Union[float, List[float]] = 4.5,
        skip_layer_strategy: Optional[SkipLayerStrategy] = None,
        skip_block_list: Optional[Union[List[List[int]], List[int]]] = None,
        stg_scale: Union[float, List[float]] = 1.0,
        rescaling_scale: Union[float, List[float]] = 0.7,
        guidance_timesteps: Optional[List[int]] = None,
        num_images_per_prompt: Optional[int] = 1,
        eta: float = 0.0,
        generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
        latents: Optional[torch.FloatTensor] = None,
        prompt_embeds: Optional[torch.FloatTensor] = None,
        prompt_attention_mask: Optional[torch.FloatTensor] = None,
        negative_prompt_embeds: Optional[torch.FloatTensor] = None,
        negative_prompt_attention_mask: Optional[torch.FloatTensor] = None,
        output_type: Optional[str] = "pil",
        return_dict: bool = True,
        callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
        conditioning_items: Optional[List[ConditioningItem]] = None,
        decode_timestep: Union[List[float], float] = 0.0,
        decode_noise_scale: Optional[List[float]] = None,
        mixed_precision: bool = False,
        offload_to_cpu: bool = False,
        enhance_prompt: bool = False,
        text_encoder_max_tokens: int = 256,
        stochastic_sampling: bool = False,
        media_items: Optional[torch.Tensor] = None,
        strength: Optional[float] = 1.0,
        skip_initial_inference_steps: int = 0,
        skip_final_inference_steps: int = 0,
        joint_pass: bool = False,
        pass_no: int = -1,
        ltxv_model=None,
        callback=None,
        *,
        stg_row_dedup: bool = True,
        dead_row_elimination: bool = True,
        latents_dtype: Optional[torch.dtype] = None,
        sample_conditioning_posterior: bool = True,
        **kwargs,
    ):
        """The reference's signature, parameter for parameter (pipeline_ltx_video.py:762-807; defaults included), and its
        behaviour for every argument the video path uses.  Read from ``**kwargs`` as the reference does (:901, :918-919):
        ``is_video``, ``vae_per_channel_normalize``, ``image_cond_noise_scale``; anything else in ``**kwargs`` (the YAML keys
        ``ltxv.py:420`` spreads into the call, ``VAE_tile_size``, ``device``, ``num_inference_steps1/2``,
        ``cfg_star_rescale`` ...) is accepted and ignored, as there.

        Returns what the reference returns: ``None`` when the transformer was interrupted, the tensor itself for
        ``return_dict=True`` (:1306), ``(tensor,)`` otherwise; ``output_type`` "latent" = (b, c, f, h, w) latents,
        "pt" = decoded video in [0, 1].

        Explicit refusals (outside this path): a string ``prompt`` (the reference's ``__call__`` does not encode it
        either: it reads ``prompt_embeds``, :1029-1051 -- ``LTXMultiScalePipeline`` / ``encode_prompt`` do), ``is_video=False``,
        ``offload_to_cpu``, ``enhance_prompt``.

        Several videos per call: b = ``prompt_embeds.shape[0] * num_images_per_prompt`` (the four prompt tensors are repeated
        per image here, prompt-major, as ``encode_prompt`` does for text).  The rows into the transformer are the
        reference's chunks [negative x b, positive x b, perturbed x b]; every sum of the guidance is per video
        (``ops.guidance_step_batched_``), so video j is what the single call with its inputs gives.  ``generator`` may be a
        list of b generators (diffusers' ``randn_tensor`` semantics); ``media_items`` and a conditioning item's clip hold b
        videos or one shared by all; all videos have one token geometry.  ``callback`` gets video 0's preview.  With sequence
        parallelism installed on the transformer b > 1 is refused.

        ``mixed_precision=True`` (:1061, :1152-1156, :1177): the latents are fp32 whatever ``prompt_embeds``' dtype is, and the
        transformer runs with ``mixed=True`` -- an fp32 residual stream between bf16 linears and attention, a bf16
        ``noise_pred``; guidance and the scheduler step update the fp32 latents.

        Keyword-only extensions behind the reference's parameters: ``stg_row_dedup`` (the STG "perturbed" row has the text
        row's inputs, so it is the text row until the step's first skipped block; those blocks run on one row less and the
        row is filled in by a copy), ``dead_row_elimination`` (rows whose guidance scale is zero at a step are not
        computed) -- both bit-identical to the plain loop; ``latents_dtype`` (default = the reference's: the dtype of
        ``prompt_embeds``, :1062); ``sample_conditioning_posterior``; and a (b, N, c) ``latents`` tensor is taken as the
        patchified initial noise as is (the reference rejects 3-D latents)."""
        is_video = kwargs.get("is_video", False)
        per_channel = kwargs.get("vae_per_channel_normalize", True)
        image_cond_noise_scale = kwargs.get("image_cond_noise_scale", 0.0)
        self.check_inputs(prompt, height, width, negative_prompt, prompt_embeds, negative_prompt_embeds,
                          prompt_attention_mask, negative_prompt_attention_mask, enhance_prompt)
        self._refuse_outside_this_path(prompt, prompt_embeds, is_video, offload_to_cpu)
        num_images = 1 if num_images_per_prompt is None else int(num_images_per_prompt)
        if num_images < 1:
            raise ValueError(f"ltxmi.LTXVideoPipeline: num_images_per_prompt={num_images_per_prompt} must be at least 1")
        if num_images > 1:
            # extension: the reference's __call__ sizes the latents by num_images_per_prompt and never repeats the prompt
            # (:905-925), which only works for one image; repeated here as encode_prompt repeats text (prompt-major)
            prompt_embeds, prompt_attention_mask = self._per_image(prompt_embeds, prompt_attention_mask, num_images)
            if negative_prompt_embeds is not None:
                negative_prompt_embeds, negative_prompt_attention_mask = self._per_image(
                    negative_prompt_embeds, negative_prompt_attention_mask, num_images)
        b = prompt_embeds.shape[0]                                                       # videos in this call
        if mixed_precision:
            # :1061: fp32 latents whatever the prompt's dtype; the transformer then keeps its residual stream in fp32 (:1177)
            if latents_dtype not in (None, torch.float32):
                raise ValueError(f"ltxmi.LTXVideoPipeline: mixed_precision=True keeps the latents in float32 "
                                 f"(pipeline_ltx_video.py:1061); latents_dtype={latents_dtype} contradicts it")
            latents_dtype = torch.float32
        tr, device = self.transformer, self._execution_device
        holder = self if ltxv_model is None else ltxv_model                              # of ``_interrupt``
        if b > 1 and getattr(tr, "_sp_interrupt", None) is not None:
            raise NotImplementedError(f"ltxmi.LTXVideoPipeline: {b} videos in one call (prompts x num_images_per_prompt) on a "
                                      "transformer with sequence parallelism installed (_sp_interrupt is set): the "
                                      "multi-GPU paths take one video per call")

        grid = (num_frames // self.video_scale_factor + 1, height // self.vae_scale_factor,
                width // self.vae_scale_factor)                                          # latent f, h, w  :921-923
        latent_shape = (b, tr.config.in_channels, *grid)
        assert strength == 1.0 or latents is not None or media_items is not None, \
            "ltxmi.LTXVideoPipeline: strength < 1 re-noises given content: pass latents or media_items with it"
        timesteps, num_inference_steps = self.retrieve_timesteps(                       # :943-952
            self.scheduler, None if timesteps is not None else num_inference_steps, device, timesteps,
            max_timestep=strength, skip_initial_inference_steps=skip_initial_inference_steps,
            skip_final_inference_steps=skip_final_inference_steps, samples_shape=latent_shape)
        if self.allowed_inference_steps is not None:                                     # :953-957
            outside = [t for t in timesteps if round(t, 4) not in self.allowed_inference_steps]
            assert not outside, f"ltxmi.LTXVideoPipeline: timesteps {outside} are not among {self.allowed_inference_steps}"
        plan = _StepPlan(tr, timesteps, guidance_scale, stg_scale, rescaling_scale, skip_block_list, guidance_timesteps,
                         (prompt_embeds, prompt_attention_mask), (negative_prompt_embeds, negative_prompt_attention_mask),
                         device, dead_row_elimination, stg_row_dedup and joint_pass, videos=b)

        start = self._initial_latents(latents, media_items, timesteps[0], latent_shape,
                                      prompt_embeds.dtype if latents_dtype is None else latents_dtype,    # :1062
                                      device, generator, per_channel)
        # conditioning items -> latents / coords / mask (+ extra tokens in front)           :1067-1085
        latents, pixel_coords, cond_mask, num_cond_latents = self.prepare_conditioning(
            conditioning_items, start.contiguous(), num_frames, height, width, per_channel, generator,
            sample_posterior=sample_conditioning_posterior)
        latents = latents.contiguous()
        init_latents = one_minus_mask = None
        if cond_mask is not None:
            init_latents, cond_mask = latents.clone(), cond_mask.contiguous()
            one_minus_mask = 1.0 - cond_mask
        # every video of a call has the same token geometry: one table (video 0's) serves all rows
        frac = pixel_coords[:1].to(torch.float32)
        frac[:, 0] = frac[:, 0] * (1.0 / frame_rate)                                     # :1086-1087
        freqs_cis = tr.precompute_freqs_cis(frac)

        if getattr(tr, "_sp_interrupt", None) is not None:          # sequence parallelism: see distributed.begin_generation
            tr._sp_interrupt.reset()
        if callback is not None:                                                         # :1100-1101
            callback(-1, None, True, override_num_inference_steps=num_inference_steps, pass_no=pass_no)

        workspace = torch.empty(b * ops.GUIDANCE_WORKSPACE_FLOATS, dtype=torch.float32, device=device)
        guidance_step_ = ops.guidance_step_ if b == 1 else ops.guidance_step_batched_
        alias_rows = {} if b == 1 else {"stg_alias_rows": b}                             # b = 1: the call as it always was
        t_dev = torch.tensor(timesteps, dtype=torch.float32, device=device)
        for i, t in enumerate(timesteps):
            if cond_mask is not None and image_cond_noise_scale > 0.0:                   # :1105-1113
                noise = _randn(latents.shape, generator, device, latents.dtype)
                ops.image_cond_noise_(latents, init_latents, noise, cond_mask, image_cond_noise_scale, t)
            use_cfg, use_stg = plan.rows(i)
            embeds, mask, nconds = plan.batch(use_cfg, use_stg)                          # nconds chunks of b rows each
            model_in = latents.to(tr.dtype)
            if nconds > 1:
                model_in = model_in.expand(nconds, -1, -1) if b == 1 else model_in.repeat(nconds, 1, 1)
            current_timestep = t_dev[i].expand(nconds * b).unsqueeze(-1)                 # [B_eff, 1]
            if cond_mask is not None:                                                    # :1145-1150, [B_eff, N]
                per_row = one_minus_mask.expand(nconds, -1) if b == 1 else one_minus_mask.repeat(nconds, 1)
                current_timestep = torch.minimum(current_timestep, per_row)
            noise_pred = tr(model_in, freqs_cis=freqs_cis, encoder_hidden_states=embeds,
                            encoder_attention_mask=mask, timestep=current_timestep,
                            stg_alias_blocks=plan.stg_alias_blocks(i, use_stg),
                            skip_layer_mask=plan.skip_mask(i, use_stg, nconds),
                            skip_layer_strategy=skip_layer_strategy, latent_shape=grid, joint_pass=joint_pass,
                            ltxv_model=holder, mixed=mixed_precision, return_dict=False, **alias_rows)[0]
            if noise_pred is None:                                                       # :1180-1181
                return None
            dt = self.scheduler.host_dt(t)
            guidance = (plan.gs[i], plan.stg[i], plan.rs[i], use_cfg, use_stg, plan.do_rescale, workspace)
            if stochastic_sampling:
                self._stochastic_step_(noise_pred, latents, t, dt, guidance, cond_mask, one_minus_mask)
            else:
                guidance_step_(noise_pred, latents, dt, *guidance, cond_mask=cond_mask, t=t)   # :1183-1241, 1309-1342
            if callback is not None:                                                     # :1243-1247: video 0's preview
                preview = latents[0, num_cond_latents:].transpose(0, 1)
                callback(i, preview.reshape(preview.shape[0], *grid), False, pass_no=pass_no)
            if callback_on_step_end is not None:
                callback_on_step_end(self, i, t, {})

        latents = self.patchifier.unpatchify(latents[:, num_cond_latents:], grid[1], grid[2], latent_shape[1])   # :1258-1268
        image = self._decode(latents, output_type, is_video, per_channel, decode_timestep, decode_noise_scale)
        return image if return_dict else (image,)                                        # :1306: the bare tensor


class _StepPlan:
    """Which rows of the batch each step of the loop runs, and on what: decided on the host, once, from the per-step
    tables.  The row batches and the skip-layer masks are built when a step first needs them and then kept."""

    def __init__(self, transformer, timesteps, guidance_scale, stg_scale, rescaling_scale, skip_block_list,
                 guidance_timesteps, positive, negative, device, dead_row_elimination, stg_row_dedup, videos=1):
        self.gs, self.stg, self.rs, self.skip = LTXVideoPipeline._guidance_tables(        # :959-1013
            timesteps, guidance_scale, stg_scale, rescaling_scale, skip_block_list, guidance_timesteps)
        self.do_cfg = any(x > 1.0 for x in self.gs)
        self.do_stg = any(x > 0.0 for x in self.stg)
        self.do_rescale = any(x != 1.0 for x in self.rs)
        self.transformer, self.device = transformer, device
        self.positive, self.negative = positive, negative
        self.dead_row_elimination, self.stg_row_dedup = dead_row_elimination, stg_row_dedup
        self.videos = videos                                     # b: every chunk of the row batch holds b rows
        self._batches, self._skip_masks = {}, {}

    def rows(self, i):
        """(negative row?, STG row?) of step ``i``.  The reference keeps num_conds constant and zeroes the scales of the
        steps that should not use a guidance (:980-983); a row whose scale is zero at a step does not reach that step's
        result (:1183-1222), so it is not computed here (``dead_row_elimination``; bit-identical: every kernel computes
        a row independently of the others)."""
        if not self.dead_row_elimination:
            return self.do_cfg, self.do_stg
        return (self.do_cfg and self.gs[i] > 1.0), (self.do_stg and self.stg[i] > 0.0)

    def batch(self, use_cfg, use_stg):
        """(embeds, mask, number of chunks) in the reference's chunk order (:1035-1051): the b negative rows, the b positive
        rows, the b STG rows (= the positive ones again); the prompt tensors hold one row per video."""
        key = (use_cfg, use_stg)
        if key not in self._batches:
            (e, m), (negative_e, negative_m) = self.positive, self.negative
            m = m.to(self.device)
            if use_cfg:
                e = torch.cat([negative_e, e], dim=0)
                m = torch.cat([negative_m.to(self.device), m], dim=0)
            if use_stg:
                e = torch.cat([e, self.positive[0]], dim=0)
                m = torch.cat([m, self.positive[1].to(self.device)], dim=0)
            self._batches[key] = (e.to(device=self.device, dtype=self.transformer.dtype), m, e.shape[0] // self.videos)
        return self._batches[key]

    def skip_mask(self, i, use_stg, nconds):                                             # :1016-1026
        """[layers, nconds * b]: zero for the perturbed rows at the step's skipped blocks, one elsewhere.  The reference's
        ``create_skip_layer_mask`` zeroes rows ``ptb_index::num_conds`` (an interleaved batch) while the batch it is applied
        to is chunked (:1035-1051, :1184-1188); the two agree for one video only.  For b videos the perturbed chunk is the
        LAST b rows, and that is what is zeroed here (``create_skip_layer_mask`` itself stays the reference's)."""
        if not use_stg or self.skip is None:
            return None
        key = (tuple(self.skip[i]), nconds)
        if key not in self._skip_masks:
            tr, b = self.transformer, self.videos
            if b == 1:
                self._skip_masks[key] = tr.create_skip_layer_mask(1, nconds, nconds - 1, list(self.skip[i]))
            elif len(self.skip[i]) == 0:
                self._skip_masks[key] = None
            else:
                host = torch.ones((len(tr.transformer_blocks), nconds * b), dtype=torch.float32)
                for block in self.skip[i]:
                    host[block, (nconds - 1) * b:] = 0
                mask = host.to(device=tr.device, dtype=tr.dtype)
                mask._ltxmi_host_rows = [[float(x) for x in row] for row in host.tolist()]   # no D2H copy per forward
                self._skip_masks[key] = mask
        return self._skip_masks[key]

    def stg_alias_blocks(self, i, use_stg):
        """How many leading blocks the STG row shares with the positive row at step ``i`` (``stg_row_dedup``): all up to
        the step's first skipped block."""
        if not (self.stg_row_dedup and use_stg):
            return 0
        blocks = self.skip[i] if self.skip is not None else []
        return min(blocks) if len(blocks) > 0 else len(self.transformer.transformer_blocks)


class LTXMultiScalePipeline:
    """pipeline_ltx_video.py:1741-1905: pass 1 at the downscaled size -> latent upsampler (x2) -> AdaIN against the
    pass-1 latents -> pass 2 from the re-noised upsampled latents -> bilinear resize to the requested size.  Same call
    contract as the reference (``ltxv.py:420-445`` calls through): ``prompt`` / ``negative_prompt`` strings are encoded by
    ``video_pipeline.encode_prompt`` with the caller's T5; everything else travels in ``**kwargs``."""

    def __init__(self, video_pipeline: LTXVideoPipeline, latent_upsampler):
        self.video_pipeline, self.latent_upsampler = video_pipeline, latent_upsampler
        self.vae = video_pipeline.vae

    def _upsample_latents(self, latest_upsampler, latents):                              # :1760-1772
        from .latent_upsampler import upsample_latents
        return upsample_latents(latest_upsampler, latents, self.vae)

    def _run_pass(self, number, args, shared, overrides, **fixed):
        """One pass of the video pipeline: the shared arguments, then what the pass fixes, then the caller's
        ``first_pass`` / ``second_pass`` overrides; ``num_inference_steps<number>`` names the pass's step count."""
        call = {**shared, **fixed, "pass_no": number, **overrides}
        if f"num_inference_steps{number}" in call:                                       # :1862 (required there)
            call["num_inference_steps"] = call[f"num_inference_steps{number}"]
        return self.video_pipeline(*args, **call)

    def __call__(self, downscale_factor: float, first_pass: dict, second_pass: dict, *args: Any, **kwargs: Any) -> Any:
        from .latent_upsampler import adain_filter_latent
        vp = self.video_pipeline
        output_type, (height, width) = kwargs["output_type"], (kwargs["height"], kwargs["width"])
        small_height, small_width = (int(x * downscale_factor) // vp.vae_scale_factor * vp.vae_scale_factor
                                     for x in (height, width))                           # :1797-1800
        # extension: VAE_tile_size / ltxv_model / device / prompt may be absent (the reference raises KeyError)
        z_tile, hw_tile = kwargs.get("VAE_tile_size") or (0, 0)                          # :1806-1814
        if z_tile > 0:
            self.vae.enable_z_tiling(z_tile)
        if hw_tile > 0:
            self.vae.enable_hw_tiling()
            self.vae.set_tiling_params(hw_tile)

        shared = {k: v for k, v in kwargs.items() if k not in ("prompt", "negative_prompt")}
        if kwargs.get("prompt") is not None or shared.get("prompt_embeds") is None:     # :1833-1852
            names = ("prompt_embeds", "prompt_attention_mask", "negative_prompt_embeds", "negative_prompt_attention_mask")
            # a list of prompts and num_images_per_prompt give prompts x images rows here; the passes must not repeat them again
            shared.update(zip(names, vp.encode_prompt(kwargs.get("prompt"), True, negative_prompt=kwargs.get("negative_prompt"),
                                                      num_images_per_prompt=shared.get("num_images_per_prompt") or 1,
                                                      device=shared.get("device"), text_encoder_max_tokens=256)))
            shared["num_images_per_prompt"] = 1
        if getattr(shared.get("ltxv_model"), "_interrupt", False):
            return None

        latents = self._run_pass(1, args, shared, first_pass, output_type="latent", height=small_height,
                                 width=small_width, joint_pass=True)
        if latents is None:
            return None
        upsampled = self._upsample_latents(self.latent_upsampler, latents)               # :1869-1873
        upsampled = adain_filter_latent(latents=upsampled, reference_latents=latents)
        result = self._run_pass(2, args, shared, second_pass, latents=upsampled, output_type=output_type,
                                height=small_height * 2, width=small_width * 2, joint_pass=False)
        if result is None or output_type == "latent":
            return result
        return _resize_frames(result, height, width)                                     # :1891-1903 (host post-processing)
