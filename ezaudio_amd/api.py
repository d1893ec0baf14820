"""Public API, signature-compatible with the reference's ``api/ezaudio.py`` (EzAudio) -- the drop-in
surface B1 of SURVEY.md section 8b.  Everything on the denoising path runs in libezaudio_hip.so; T5
(``transformers``) and the VAE are pre/post models outside this round's scope, so
they can be injected; when not injected, T5 is loaded the way the reference loads it.
"""
import random
import sys
import urllib.request
from pathlib import Path

import numpy as np
import torch

from .config import configs, controlnet_configs, load_yaml_with_includes
from .denoiser import MaskDiT
from .sampler import apg_entries, canvas_windows, check_apg, check_solver, inference, inference_controlnet, loop_windows
from .scheduler import DDIMScheduler

MAX_SEED = np.iinfo(np.int32).max


class EzAudio:
    def __init__(self, model_name, ckpt_path=None, vae_path=None, device='cuda',
                 autoencoder=None, tokenizer=None, text_encoder=None, state_dict=None, native_text_encoder=False):
        self.device = device
        config_name = configs[model_name]['config']
        if ckpt_path is None and state_dict is None:
            ckpt_path = self.download_ckpt(configs[model_name])
        if vae_path is None and autoencoder is None:
            vae_path = self.download_ckpt(configs['vae'])
        (self.autoencoder, self.unet, self.tokenizer, self.text_encoder, self.noise_scheduler,
         self.params) = self.load_models(config_name, ckpt_path, vae_path, device, autoencoder, tokenizer,
                                         text_encoder, state_dict, native_text_encoder=native_text_encoder)

    def download_ckpt(self, model_dict):
        """api/ezaudio.py:44-65."""
        local_path = Path(model_dict['path'])
        url = model_dict['url']
        local_path.parent.mkdir(parents=True, exist_ok=True)
        if not local_path.exists() and url:
            print(f"Downloading from {url} to {local_path}...")

            def progress_bar(block_num, block_size, total_size):
                sys.stdout.write(f"\rProgress: {block_num * block_size / total_size * 100:.2f}%")
                sys.stdout.flush()
            try:
                urllib.request.urlretrieve(url, local_path, reporthook=progress_bar)
                print(f"Downloaded checkpoint to {local_path}")
            except Exception as e:
                # the reference prints and continues (api/ezaudio.py:61-62), which only moves the failure to a confusing
                # torch.load on a missing file: fail here, naming the URL
                raise RuntimeError(f'could not download {url} to {local_path}: {e}') from e
        else:
            print(f"Checkpoint already exists at {local_path}")
        return local_path

    def load_models(self, config_name, ckpt_path, vae_path, device, autoencoder=None, tokenizer=None,
                    text_encoder=None, state_dict=None, native_text_encoder=False):
        """api/ezaudio.py:68-99.  native_text_encoder: when no encoder is injected, the T5 weights are loaded as the reference loads them,
        converted to the HIP encoder (ezaudio_amd/t5.py) and the transformers model is released."""
        params = load_yaml_with_includes(config_name)
        if autoencoder is None:   # api/ezaudio.py:75-79; an injected callable with the same surface is also accepted
            from .vae import Autoencoder
            autoencoder = Autoencoder(ckpt_path=vae_path, model_type=params['autoencoder']['name'],
                                      quantization_first=params['autoencoder']['q_first'], device=device)
        if tokenizer is None or text_encoder is None:
            from transformers import T5EncoderModel, T5Tokenizer
            tokenizer = T5Tokenizer.from_pretrained(params['text_encoder']['model'])
            text_encoder = T5EncoderModel.from_pretrained(params['text_encoder']['model'])
            if native_text_encoder:
                from .t5 import T5Encoder
                hf, text_encoder = text_encoder, None
                text_encoder = T5Encoder.from_hf(hf, device, max_len=max(512, int(params['text_encoder']['max_length'])))
                del hf
            else:
                text_encoder = text_encoder.to(device)
            text_encoder.eval()
        unet = MaskDiT(device=device, **params['model'])
        if state_dict is None:
            state_dict = torch.load(ckpt_path, map_location='cpu')['model']
        unet.load_state_dict(state_dict)
        unet.eval()
        noise_scheduler = DDIMScheduler(**params['diff'])
        return autoencoder, unet, tokenizer, text_encoder, noise_scheduler, params

    def _window_radius(self, attention_window):
        """Seconds (the full span a frame sees) -> radius in latent frames for sampler.inference; None stays None."""
        if attention_window is None:
            return None
        if isinstance(attention_window, (list, tuple)):
            raise ValueError('attention_window is one value per call: the prompts of a call share the attention kernels')
        if isinstance(attention_window, bool) or not attention_window > 0:
            raise ValueError(f'attention_window is a span in seconds > 0, got {attention_window!r}')
        radius = int(round(attention_window * self.params['autoencoder']['latent_sr'] / 2))
        if radius < 1:
            raise ValueError(f'attention_window of {attention_window} s is less than one latent frame on either side')
        return radius

    @staticmethod
    def _apg_kw(apg, text, guidance_scale, guidance_rescale):
        """`apg` of a request as the keyword inference() takes, refused here -- before anything is encoded -- where the request cannot have it."""
        if apg is None or apg is False:
            return {}
        texts = [text] if isinstance(text, str) else list(text)
        n = len(texts)
        if isinstance(apg, (list, tuple)) and (isinstance(text, str) or len(apg) != n):
            raise ValueError('a list of apg entries needs a list of prompts of the same size: True, a dict, or None, per prompt')
        per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n   # noqa: E731
        check_apg(apg_entries(apg, n), [None if t == '' else g for t, g in zip(texts, per(guidance_scale))], per(guidance_rescale))
        return dict(apg=apg)

    def generate_audio(self, text, length=10, guidance_scale=5, guidance_rescale=0.75, ddim_steps=100, eta=1,
                       random_seed=None, randomize_seed=False, attention_window=None, compose=None, emphasis=False, apg=None, solver='ddim'):
        """`emphasis=True` reads '(words:1.6)' markup in the prompts (sampler.parse_emphasis: per-token weights in cross-attention; the default leaves every prompt
        verbatim; audio quality on the real checkpoints is unmeasured) -- here and on editing_audio, audio_to_audio, generate_long_audio and generate_loop.
        api/ezaudio.py:101-130.  `text` may also be a list of prompts (batched extension): the result is then
        an array [N, T].  With a list of prompts `length` may be a list too, one duration in seconds per prompt (mixed-length
        batch, one call): the result is then (sr, [one 1-D array per prompt]), each trimmed to its own duration.
        `guidance_scale`, `guidance_rescale`, `eta` and `random_seed` may be lists as well, one entry per prompt of the list `text`: every
        prompt is sampled as the call with it alone would sample it (return shapes unchanged).  A prompt '' inside a list runs without
        guidance (the "empty input" rule per prompt); `randomize_seed` draws one seed per prompt of a list.
        `solver='dpmpp_2m'` samples with DPM-Solver++(2M) instead of DDIM; it is deterministic, so pass eta=0 with it (the default eta=1
        raises).  Quality at reduced `ddim_steps` on the real checkpoints is unmeasured.
        `attention_window` (seconds; one value): sliding-window self-attention -- every latent frame attends to the frames inside a span of that many seconds
        centred on it (radius round(seconds * latent_sr / 2) frames), so a `length` beyond the trained 10 s keeps every pair of frames inside the trained range
        of relative positions: attention_window=10 gives each frame the 501 keys of the trained row.  A span that covers the clip is the plain call, bit for
        bit.  Audio quality of windowed sampling on the real checkpoints is unmeasured.
        `compose` (composed guidance): further prompts with weights next to `text`, each guided against the empty prompt with its own weight -- "both sounds
        must be there, and less of that one": compose=[('distant thunder', 0.8), ('wind', -0.5)].  `text` has weight 1 and is the reference of the guidance
        rescale; a negative weight steers away from its prompt.  With a list of prompts, one such list (or None) per prompt.  The batch grows to K + 1 rows per
        prompt.  ValueError for a prompt list of another size, a non-finite weight, more than 7 extra prompts, or a call without guidance (text '').  No extra
        prompt is the plain call, bit for bit.  Audio quality on the real checkpoints -- which weights sound like "both" or "less of" -- is unmeasured.
        `apg` (adaptive projected guidance, Sadat et al.; also on editing_audio and audio_to_audio): guidance that does not over-drive the latent at the scales
        that make a prompt stick.  apg=True, or apg=dict(eta=0.0, norm_threshold=0.0, momentum=-0.5) with any of the three keys; with a list of prompts also one
        entry (or None) per prompt.  The guidance direction loses its component parallel to the prediction (`eta`: the share that stays), carries `momentum`
        across steps and is capped at `norm_threshold` (0: no cap).  True means eta 0, momentum -0.5 and NO cap: which cap suits the EzAudio latent is
        unmeasured, so none is invented.  The guidance rescale is not applied to it: pass guidance_rescale=0 with apg (the default 0.75 raises), or a list with 0
        for the prompts that take it.  ValueError also with `compose`, for text '' (no guidance), an unknown key, a non-finite value or a negative cap.
        Which settings sound best on the real checkpoints is unmeasured."""
        neg_text = None
        apg_kw = self._apg_kw(apg, text, guidance_scale, guidance_rescale)
        if compose is not None and not isinstance(text, str) and len(compose) != len(text):
            raise ValueError('compose for a list of prompts is a list of the same size: one list of (text, weight) pairs, or None, per prompt')
        check_solver(solver, eta)
        radius = self._window_radius(attention_window)
        for name, v in (('guidance_scale', guidance_scale), ('guidance_rescale', guidance_rescale), ('eta', eta), ('random_seed', random_seed)):
            if isinstance(v, (list, tuple)) and (isinstance(text, str) or len(v) != len(text)):
                raise ValueError(f'a list of {name} needs a list of prompts of the same size')
        if isinstance(ddim_steps, (list, tuple)):
            raise ValueError('ddim_steps must be one value per call: per-prompt step counts are not supported')
        latent_sr = self.params['autoencoder']['latent_sr']
        per_prompt = isinstance(length, (list, tuple))
        if per_prompt:
            if isinstance(text, str) or len(length) != len(text):
                raise ValueError('a list of lengths needs a list of prompts of the same size')
            length = [int(round(v * latent_sr)) for v in length]
        else:
            length = length * latent_sr
        gt, gt_mask = None, None
        if text == '':
            guidance_scale = None
            print('empty input')
        elif not isinstance(text, str) and '' in text:
            gs = list(guidance_scale) if isinstance(guidance_scale, (list, tuple)) else [guidance_scale] * len(text)
            guidance_scale = [None if t == '' else g for t, g in zip(text, gs)]
            print('empty input')
        if randomize_seed:
            random_seed = random.randint(0, MAX_SEED) if isinstance(text, str) else [random.randint(0, MAX_SEED) for _ in text]
        pred = inference(self.autoencoder, self.unet, gt, gt_mask, self.tokenizer, self.text_encoder, self.params,
                         self.noise_scheduler, text, neg_text, length, guidance_scale, guidance_rescale, ddim_steps,
                         eta, random_seed, self.device, solver=solver, attention_window=radius, **({} if compose is None else dict(compose=compose)), **({} if not emphasis else dict(emphasis=True)), **apg_kw)
        pred = pred.cpu().numpy()
        if per_prompt:
            ratio = self.params['autoencoder']['sr'] // latent_sr
            return self.params['autoencoder']['sr'], [pred[i, 0, :n * ratio] for i, n in enumerate(length)]
        pred = pred.squeeze(0).squeeze(0) if isinstance(text, str) or len(text) == 1 else pred.squeeze(1)
        return self.params['autoencoder']['sr'], pred

    def generate_scene(self, scene, length, crossfade=1.0, guidance_scale=5, guidance_rescale=0.75, ddim_steps=100, eta=1, random_seed=None,
                       randomize_seed=False, attention_window=None, solver='ddim'):
        """ONE clip of `length` seconds whose prompt changes over time (prompt timeline): `scene` is a list of (text, start_s, end_s[, weight]) entries, which
        may overlap; every latent frame weights the entries by their trapezoid envelopes (`crossfade` seconds per edge, sampler.scene_weights) in every block's
        cross-attention, so prompts switch, cross-fade or mix inside the one sample.  Returns (sr, waveform).  A scene of one entry is generate_audio of that
        text.  The other arguments as in generate_audio (one value each).  ValueError as scene_weights: an uncovered frame, an entry outside the clip, more than
        16 entries.  Audio quality on the real checkpoints -- whether a cross-fade of the softmax prior sounds like one, which fade length to choose -- is unmeasured."""
        from .sampler import scene_weights
        latent_sr = self.params['autoencoder']['latent_sr']
        frames = int(round(length * latent_sr))
        prompts, weights = scene_weights(scene, frames, latent_sr, crossfade)
        if len(prompts) == 1:
            return self.generate_audio(prompts[0], length, guidance_scale, guidance_rescale, ddim_steps, eta, random_seed, randomize_seed,
                                       attention_window=attention_window, solver=solver)
        check_solver(solver, eta)
        radius = self._window_radius(attention_window)
        for name, v in (('guidance_scale', guidance_scale), ('guidance_rescale', guidance_rescale), ('eta', eta), ('random_seed', random_seed)):
            if isinstance(v, (list, tuple)):
                raise ValueError(f'a scene is one clip: one {name}')
        if randomize_seed:
            random_seed = random.randint(0, MAX_SEED)
        pred = inference(self.autoencoder, self.unet, None, None, self.tokenizer, self.text_encoder, self.params, self.noise_scheduler, [prompts], None,
                         frames, guidance_scale, guidance_rescale, ddim_steps, eta, random_seed, self.device, solver=solver, attention_window=radius,
                         prompt_weights=[weights])
        return self.params['autoencoder']['sr'], pred.cpu().numpy().squeeze(0).squeeze(0)

    def generate_long_audio(self, text, length, window=10, overlap=2.5, guidance_scale=5, guidance_rescale=0.75, ddim_steps=100, eta=1,
                            random_seed=None, randomize_seed=False, solver='ddim', emphasis=False):
        """A clip of `length` seconds, longer than the `window` seconds the model was trained on: the latent canvas is covered by overlapping windows of
        `window` seconds that share at least `overlap` seconds with their neighbours (sampler.canvas_windows chooses the fewest such windows, spread evenly),
        all windows are denoised together as the prompts of ONE batched sampler call, the shared frames are cross-faded inside every step, and the canvas is
        decoded in one call.  Returns (sr, waveform [T]) like generate_audio.
        `text` is one prompt for the whole clip, or a list with one prompt per window -- a scene that changes over time.  The settings are scalars.
        `length <= window` is generate_audio(text, length, ...): the same call, the same result.
        Audio quality on the real checkpoints (seam audibility, the choice of overlap, the comparison with generate_audio(length=...) as one long row) is
        unmeasured."""
        latent_sr = self.params['autoencoder']['latent_sr']
        if isinstance(length, (list, tuple)):
            raise ValueError('generate_long_audio makes one clip: length is one duration in seconds')
        offsets, frames = canvas_windows(int(round(length * latent_sr)), int(round(window * latent_sr)), int(round(overlap * latent_sr)))
        n_win = len(offsets)
        if not isinstance(text, str) and len(text) != n_win:
            raise ValueError(f'{len(text)} prompts for {n_win} windows ({length} s in windows of {window} s that share {overlap} s): one prompt, or one per window')
        if n_win == 1:
            return self.generate_audio(text if isinstance(text, str) else text[0], length, guidance_scale, guidance_rescale, ddim_steps, eta, random_seed,
                                       randomize_seed, solver=solver)
        check_solver(solver, eta)
        for name, v in (('guidance_scale', guidance_scale), ('guidance_rescale', guidance_rescale), ('eta', eta), ('random_seed', random_seed),
                        ('ddim_steps', ddim_steps)):
            if isinstance(v, (list, tuple)):
                raise ValueError(f'generate_long_audio takes one {name} for the whole clip')
        prompts = [text] * n_win if isinstance(text, str) else list(text)
        if all(t == '' for t in prompts):
            guidance_scale = None
            print('empty input')
        if randomize_seed:
            random_seed = random.randint(0, MAX_SEED)
        pred = inference(self.autoencoder, self.unet, None, None, self.tokenizer, self.text_encoder, self.params, self.noise_scheduler, prompts, None,
                         frames, guidance_scale, guidance_rescale, ddim_steps, eta, random_seed, self.device, canvas_offsets=offsets, solver=solver, **({} if not emphasis else dict(emphasis=True)))
        return self.params['autoencoder']['sr'], pred.cpu().numpy().squeeze(0).squeeze(0)

    def generate_loop(self, text, length, window=10, overlap=2.5, guidance_scale=5, guidance_rescale=0.75, ddim_steps=100, eta=1,
                      random_seed=None, randomize_seed=False, solver='ddim', decode_context=None, emphasis=False):
        """A clip of `length` seconds that runs from its end into its own beginning: ``np.tile(waveform, k)`` is the loop.  The latent canvas is a RING covered
        by windows of `window` seconds, each sharing at least `overlap` seconds with the next one around the ring, the last with the first
        (sampler.loop_windows chooses the fewest such windows, at least two, spread evenly); all windows are denoised together as the prompts of ONE batched
        sampler call, the shared frames are cross-faded inside every step, and the ring is decoded in one call with wrapped context in place of the VAE's zero
        halos (sampler.decode_circular; `decode_context` latent frames, None = the decoder's receptive field).  Returns (sr, waveform [T]).
        `text` is one prompt for the whole loop, or a list with one prompt per window.  The settings are scalars.  Any `length` of at least 2 latent frames
        is valid: a loop no longer than the window is two windows of its own length, half a turn apart.
        Audio quality on the real checkpoints (whether the seam is audible, the choice of overlap and ramp) is unmeasured."""
        latent_sr = self.params['autoencoder']['latent_sr']
        if isinstance(length, (list, tuple)):
            raise ValueError('generate_loop makes one clip: length is one duration in seconds')
        ring, win, shared = int(round(length * latent_sr)), int(round(window * latent_sr)), int(round(overlap * latent_sr))
        if shared < 0 or shared >= win:
            raise ValueError(f'overlap={overlap} outside [0, window = {window})')
        if ring <= win:   # two windows of the loop's own length share half a turn with each other, whatever was asked of the full window
            shared = min(shared, ring // 2)
        offsets, frames = loop_windows(ring, win, shared)
        n_win = len(offsets)
        if not isinstance(text, str) and len(text) != n_win:
            raise ValueError(f'{len(text)} prompts for {n_win} windows (a loop of {length} s in windows of {window} s that share {overlap} s): one prompt, or one per window')
        check_solver(solver, eta)
        for name, v in (('guidance_scale', guidance_scale), ('guidance_rescale', guidance_rescale), ('eta', eta), ('random_seed', random_seed),
                        ('ddim_steps', ddim_steps)):
            if isinstance(v, (list, tuple)):
                raise ValueError(f'generate_loop takes one {name} for the whole clip')
        prompts = [text] * n_win if isinstance(text, str) else list(text)
        if all(t == '' for t in prompts):
            guidance_scale = None
            print('empty input')
        if randomize_seed:
            random_seed = random.randint(0, MAX_SEED)
        pred = inference(self.autoencoder, self.unet, None, None, self.tokenizer, self.text_encoder, self.params, self.noise_scheduler, prompts, None,
                         frames, guidance_scale, guidance_rescale, ddim_steps, eta, random_seed, self.device, canvas_offsets=offsets, canvas_loop=ring,
                         decode_context=decode_context, solver=solver, **({} if not emphasis else dict(emphasis=True)))
        return self.params['autoencoder']['sr'], pred.cpu().numpy().squeeze(0).squeeze(0)

    def _load_edit_clip(self, gt_file):
        """The recording of an edit, peak-normalised (api/ezaudio.py:143-144): a path (librosa) or a 1-D numpy waveform at the model's sample rate."""
        sr = self.params['autoencoder']['sr']
        if isinstance(gt_file, np.ndarray):
            if gt_file.ndim != 1:
                raise ValueError(f'a waveform must be 1-D, got shape {gt_file.shape}')
            gt = gt_file.astype(np.float32)
        else:
            import librosa
            gt, _ = librosa.load(gt_file, sr=sr)
        return gt / (np.max(np.abs(gt)) + 1e-9)

    def _edit_request(self, gt, boundary, mask_start, mask_length):
        """The crop / pad / mask bookkeeping of ONE edit (api/ezaudio.py:145-157) on a normalised recording `gt`: the recording the result is pasted into
        (padded behind when the mask runs past its end), the chunk that is re-synthesised (samples [lo, hi) of it), the mask inside the chunk in seconds,
        and the chunk's duration.  The single and the batched form share it, so they share its arithmetic."""
        sr = self.params['autoencoder']['sr']
        mask_end = mask_start + mask_length
        audio_length = len(gt) / sr
        mask_start = min(mask_start, audio_length)
        if mask_end > audio_length:  # out-padding mode
            gt = np.pad(gt, (0, round((mask_end - audio_length) * sr)), 'constant')
            audio_length = len(gt) / sr
        output_audio = gt.copy()
        boundary = min((mask_end - mask_start) / 2, boundary)
        start_idx = max(mask_start - boundary, 0)
        end_idx = min(mask_end + boundary, audio_length)
        mask_start -= start_idx
        mask_end -= start_idx
        lo, hi = round(start_idx * sr), round(end_idx * sr)
        return dict(output_audio=output_audio, chunk=gt[lo:hi], lo=lo, hi=hi, mask_start=mask_start, mask_end=mask_end,
                    chunk_length=end_idx - start_idx)

    def editing_audio(self, text, boundary, gt_file, mask_start, mask_length, guidance_scale=3.5, guidance_rescale=0,
                      ddim_steps=100, eta=1, random_seed=None, randomize_seed=False, attention_window=None, emphasis=False, apg=None, solver='ddim'):
        """api/ezaudio.py:132-207 (crop / pad / mask bookkeeping on the host, sampling on the GPU).  `solver`, `apg` and `attention_window` (seconds; quality on the real
        checkpoints unmeasured) as in generate_audio.  `gt_file` is a path or a
        1-D numpy waveform at the model's sample rate.

        Batched extension: `text` may be a list of prompts, one edit per entry in ONE encode, ONE sampler call and ONE decode; the result is then
        (sr, [one 1-D array per request]), each its own normalised recording with its own chunk pasted in, as the single call returns it.  `gt_file` is then
        a list of the same size, or one recording for every request (loaded once, cropped per request).  `boundary`, `mask_start`, `mask_length`,
        `guidance_scale`, `guidance_rescale`, `eta` and `random_seed` may each be one value or a list with one entry per request; `ddim_steps` stays one
        value.  A prompt '' inside a list runs without guidance; `randomize_seed` draws one seed per request.  The VAE bottleneck's noise is drawn per clip
        from the global generator, in list order: the draws the single calls in that order make.  The autoencoder must take `lengths=` and have
        `latent_lengths` (this package's Autoencoder does)."""
        check_solver(solver, eta)
        radius = self._window_radius(attention_window)
        apg_kw = self._apg_kw(apg, text, guidance_scale, guidance_rescale)
        if not isinstance(text, str):
            return self._editing_audio_batch(list(text), boundary, gt_file, mask_start, mask_length, guidance_scale, guidance_rescale, ddim_steps, eta,
                                             random_seed, randomize_seed, solver, radius, emphasis, apg_kw)
        for name, v in (('gt_file', gt_file), ('boundary', boundary), ('mask_start', mask_start), ('mask_length', mask_length),
                        ('guidance_scale', guidance_scale), ('guidance_rescale', guidance_rescale), ('eta', eta), ('random_seed', random_seed)):
            if isinstance(v, (list, tuple)):
                raise ValueError(f'a list of {name} needs a list of prompts of the same size')
        if isinstance(ddim_steps, (list, tuple)):
            raise ValueError('ddim_steps must be one value per call: per-prompt step counts are not supported')
        neg_text = None
        if text == '':
            guidance_scale = None
            print('empty input')
        sr = self.params['autoencoder']['sr']
        latent_sr = self.params['autoencoder']['latent_sr']
        req = self._edit_request(self._load_edit_clip(gt_file), boundary, mask_start, mask_length)
        gt = torch.tensor(req['chunk']).unsqueeze(0).unsqueeze(1).to(self.device)
        gt_latent = self.autoencoder(audio=gt)
        B, D, L = gt_latent.shape
        gt_mask = torch.zeros(B, D, L).to(self.device)
        gt_mask[:, :, round(req['mask_start'] * latent_sr): round(req['mask_end'] * latent_sr)] = 1
        gt_mask = gt_mask.bool()
        if randomize_seed:
            random_seed = random.randint(0, MAX_SEED)
        pred = inference(self.autoencoder, self.unet, gt_latent, gt_mask, self.tokenizer, self.text_encoder,
                         self.params, self.noise_scheduler, text, neg_text, L, guidance_scale, guidance_rescale,
                         ddim_steps, eta, random_seed, self.device, solver=solver, attention_window=radius, **({} if not emphasis else dict(emphasis=True)), **apg_kw)
        pred = pred.cpu().numpy().squeeze(0).squeeze(0)
        pred = pred[:round(req['chunk_length'] * sr)]
        output_audio = req['output_audio']
        output_audio[req['lo']:req['hi']] = pred
        return sr, output_audio

    def _editing_audio_batch(self, text, boundary, gt_file, mask_start, mask_length, guidance_scale, guidance_rescale, ddim_steps, eta, random_seed,
                             randomize_seed, solver, radius=None, emphasis=False, apg_kw=None):
        """editing_audio for a list of prompts: N crops in one ragged encode, one sampler call at per-request latent lengths, one ragged decode."""
        n = len(text)
        if isinstance(ddim_steps, (list, tuple)):
            raise ValueError('ddim_steps must be one value per call: per-prompt step counts are not supported')
        for name, v in (('gt_file', gt_file), ('boundary', boundary), ('mask_start', mask_start), ('mask_length', mask_length),
                        ('guidance_scale', guidance_scale), ('guidance_rescale', guidance_rescale), ('eta', eta), ('random_seed', random_seed)):
            if isinstance(v, (list, tuple)) and len(v) != n:
                raise ValueError(f'a list of {name} needs a list of prompts of the same size')
        if n == 0:
            raise ValueError('a list of prompts needs at least one prompt')
        if not hasattr(self.autoencoder, 'latent_lengths'):
            raise NotImplementedError('a batched edit needs an autoencoder that takes lengths= and has latent_lengths (ezaudio_amd.vae.Autoencoder)')
        per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n   # noqa: E731
        sr = self.params['autoencoder']['sr']
        latent_sr = self.params['autoencoder']['latent_sr']
        if isinstance(gt_file, (list, tuple)):
            clips = [self._load_edit_clip(f) for f in gt_file]
        else:
            clips = [self._load_edit_clip(gt_file)] * n                         # one recording for every request: loaded once, cropped per request
        reqs = [self._edit_request(c, b, ms, ml) for c, b, ms, ml in zip(clips, per(boundary), per(mask_start), per(mask_length))]
        if '' in text:
            guidance_scale = [None if t == '' else g for t, g in zip(text, per(guidance_scale))]
            print('empty input')
        samples = [len(r['chunk']) for r in reqs]
        wav = torch.zeros(n, 1, max(samples))
        for i, r in enumerate(reqs):
            wav[i, 0, :samples[i]] = torch.from_numpy(r['chunk'])
        gt_latent = self.autoencoder(audio=wav.to(self.device), lengths=samples)
        frames = [int(v) for v in self.autoencoder.latent_lengths(samples)]
        _, D, L = gt_latent.shape
        gt_mask = torch.zeros(n, D, L)
        for i, r in enumerate(reqs):   # each clip's mask at its own latent length, nothing beyond
            gt_mask[i, :, min(round(r['mask_start'] * latent_sr), frames[i]):min(round(r['mask_end'] * latent_sr), frames[i])] = 1
        gt_mask = gt_mask.to(self.device).bool()
        if randomize_seed:
            random_seed = [random.randint(0, MAX_SEED) for _ in text]
        pred = inference(self.autoencoder, self.unet, gt_latent, gt_mask, self.tokenizer, self.text_encoder,
                         self.params, self.noise_scheduler, text, None, frames, guidance_scale, guidance_rescale,
                         ddim_steps, eta, random_seed, self.device, solver=solver, attention_window=radius, **({} if not emphasis else dict(emphasis=True)), **(apg_kw or {}))
        pred = pred.cpu().numpy()
        outs = []
        for i, r in enumerate(reqs):
            out = r['output_audio']
            out[r['lo']:r['hi']] = pred[i, 0, :round(r['chunk_length'] * sr)]
            outs.append(out)
        return sr, outs

    def audio_to_audio(self, text, audio, strength=0.5, guidance_scale=5, guidance_rescale=0.75, ddim_steps=100, eta=1, random_seed=None,
                       randomize_seed=False, attention_window=None, solver='ddim', emphasis=False, apg=None):
        """Re-render a recording under a prompt, staying as close to it as `strength` says (not in the reference: the standard "start the sampler from the
        noised clip" of image-to-image, SDEdit).  `audio` is a path or a 1-D numpy waveform at the model's sample rate, peak-normalised and encoded whole;
        `strength` in (0, 1] is the share of the `ddim_steps` that are run (scheduler.start_step): 1 starts from pure noise, the plain generate_audio of the
        clip's length, small values change little.  Returns (sr, waveform) of latent_frames * ratio samples.  `solver` and `apg` as in generate_audio.

        Batched extension: `text` may be a list of prompts, one request per entry in ONE ragged encode, ONE sampler call and ONE ragged decode; the result is
        then (sr, [one 1-D array per request]).  `audio` is then a list of the same size, or one clip shared by all requests; `strength`, `guidance_scale`,
        `guidance_rescale`, `eta` and `random_seed` may each be one value or a list with one entry per request; `ddim_steps` stays one value.  A prompt ''
        inside a list runs without guidance; `randomize_seed` draws one seed per request.  The autoencoder must take `lengths=` and have `latent_lengths`
        (this package's Autoencoder does).

        `attention_window` (seconds) as in generate_audio: a recording longer than the trained 10 s sampled with sliding-window self-attention.

        Audio quality versus strength, and of windowed sampling, on the real checkpoints is unmeasured."""
        check_solver(solver, eta)
        radius = self._window_radius(attention_window)
        apg_kw = self._apg_kw(apg, text, guidance_scale, guidance_rescale)
        if isinstance(ddim_steps, (list, tuple)):
            raise ValueError('ddim_steps must be one value per call: per-prompt step counts are not supported')
        sr = self.params['autoencoder']['sr']
        ratio = sr // self.params['autoencoder']['latent_sr']
        batched = not isinstance(text, str)
        n = len(text) if batched else 1
        for name, v in (('audio', audio), ('strength', strength), ('guidance_scale', guidance_scale), ('guidance_rescale', guidance_rescale), ('eta', eta),
                        ('random_seed', random_seed)):
            if isinstance(v, (list, tuple)) and (not batched or len(v) != n):
                raise ValueError(f'a list of {name} needs a list of prompts of the same size')
        if batched and n == 0:
            raise ValueError('a list of prompts needs at least one prompt')
        per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n   # noqa: E731
        self.noise_scheduler.set_timesteps(ddim_steps)
        for s in per(strength):
            self.noise_scheduler.start_step(s)   # a strength outside (0, 1], or one that leaves no step to run, raises before anything is encoded
        if batched and not hasattr(self.autoencoder, 'latent_lengths'):
            raise NotImplementedError('a batched audio_to_audio needs an autoencoder that takes lengths= and has latent_lengths (ezaudio_amd.vae.Autoencoder)')
        if isinstance(audio, (list, tuple)):
            clips = [self._load_edit_clip(a) for a in audio]
        else:
            clips = [self._load_edit_clip(audio)] * n                          # one clip for every request: loaded once
        # (the autoencoder's own samples-per-frame where it tells: an injected one need not have the ratio of the yml)
        n_frames = self.autoencoder.latent_lengths if hasattr(self.autoencoder, 'latent_lengths') else (lambda ns: [v // ratio for v in ns])
        for c in clips:
            if n_frames([len(c)])[0] < 1:
                raise ValueError(f'a clip of {len(c)} samples is shorter than one latent frame')
        if not batched:
            if text == '':
                guidance_scale = None
                print('empty input')
            if randomize_seed:
                random_seed = random.randint(0, MAX_SEED)
            wav = torch.tensor(clips[0]).unsqueeze(0).unsqueeze(1).to(self.device)
            latent = self.autoencoder(audio=wav)
            L = latent.shape[-1]
            pred = inference(self.autoencoder, self.unet, None, None, self.tokenizer, self.text_encoder, self.params, self.noise_scheduler, text, None, L,
                             guidance_scale, guidance_rescale, ddim_steps, eta, random_seed, self.device, solver=solver, init_latents=latent,
                             strength=strength, attention_window=radius, **({} if not emphasis else dict(emphasis=True)), **apg_kw)
            return sr, pred.cpu().numpy().squeeze(0).squeeze(0)
        text = list(text)
        if '' in text:
            guidance_scale = [None if t == '' else g for t, g in zip(text, per(guidance_scale))]
            print('empty input')
        if randomize_seed:
            random_seed = [random.randint(0, MAX_SEED) for _ in text]
        samples = [len(c) for c in clips]
        wav = torch.zeros(n, 1, max(samples))
        for i, c in enumerate(clips):
            wav[i, 0, :samples[i]] = torch.from_numpy(c)
        latent = self.autoencoder(audio=wav.to(self.device), lengths=samples)
        frames = [int(v) for v in self.autoencoder.latent_lengths(samples)]
        pred = inference(self.autoencoder, self.unet, None, None, self.tokenizer, self.text_encoder, self.params, self.noise_scheduler, text, None, frames,
                         guidance_scale, guidance_rescale, ddim_steps, eta, random_seed, self.device, solver=solver, init_latents=latent,
                         strength=per(strength), attention_window=radius, **({} if not emphasis else dict(emphasis=True)), **apg_kw)
        pred = pred.cpu().numpy()
        up = pred.shape[-1] // max(frames)                                     # samples per latent frame, as decoded
        return sr, [pred[i, 0, :f * up] for i, f in enumerate(frames)]


class EzAudio_ControlNet(EzAudio):
    """api/controlnet.py:31-160: EzAudio-L + energy ControlNet (``model_name='energy'``)."""

    def __init__(self, model_name, ckpt_path=None, controlnet_path=None, vae_path=None, device='cuda', autoencoder=None,
                 tokenizer=None, text_encoder=None, state_dict=None, controlnet_state_dict=None, native_text_encoder=False):
        self.device = device
        config_name = controlnet_configs[model_name]['config']
        if ckpt_path is None and state_dict is None:
            ckpt_path = self.download_ckpt(controlnet_configs['model'])
        if controlnet_path is None and controlnet_state_dict is None:
            controlnet_path = self.download_ckpt(controlnet_configs[model_name])
        if vae_path is None and autoencoder is None:
            vae_path = self.download_ckpt(controlnet_configs['vae'])
        (self.autoencoder, self.unet, self.tokenizer, self.text_encoder, self.noise_scheduler,
         self.params) = self.load_models(config_name, ckpt_path, vae_path, device, autoencoder, tokenizer, text_encoder,
                                         state_dict, native_text_encoder=native_text_encoder)
        from .conditions import Conditioner
        from .controlnet import DiTControlNet
        cfg = self.params['model'].copy()
        cfg.update(self.params['controlnet'])                      # api/controlnet.py:92-95
        self.controlnet = DiTControlNet(device=device, **cfg)
        if controlnet_state_dict is None:
            controlnet_state_dict = torch.load(controlnet_path, map_location='cpu')['model']
        self.controlnet.load_state_dict(controlnet_state_dict)
        self.conditioner = Conditioner(**self.params['conditioner'])

    def _load_clip(self, audio, surpass_noise, seconds):
        """One reference recording as the reference prepares it (api/controlnet.py:118-127): peak-normalised, gated, padded or cut to `seconds`.
        `audio` is a path (librosa) or a 1-D numpy waveform at the model's sample rate.  Returns (waveform, its length before padding / cutting)."""
        sr = self.params['autoencoder']['sr']
        if isinstance(audio, np.ndarray):
            if audio.ndim != 1:
                raise ValueError(f'a waveform must be 1-D, got shape {audio.shape}')
            gt = audio.astype(np.float32)
        else:
            import librosa
            gt, _ = librosa.load(audio, sr=sr)
        gt = gt / (np.max(np.abs(gt)) + 1e-9)
        if surpass_noise > 0:
            gt[np.abs(gt) <= surpass_noise] = 0
        original_length = len(gt)
        num_samples = int(round(seconds * sr))
        gt = np.pad(gt, (0, num_samples - len(gt)), 'constant') if len(gt) < num_samples else gt[:num_samples]
        return gt, original_length

    def generate_audio(self, text, audio_path, surpass_noise=0, guidance_scale=3.5, guidance_rescale=0, ddim_steps=50,
                       eta=1, conditioning_scale=1, random_seed=None, randomize_seed=False, length=None, solver='ddim'):
        """api/controlnet.py:113-160: the control curve is the frame energy of a reference recording.  `solver` as in EzAudio.generate_audio.

        Batched extension: `text` and `audio_path` may be lists of equal size (an `audio_path` entry is a file or a 1-D numpy waveform at the model's
        sample rate), one energy-controlled request per entry in ONE sampler call; the result is then (sr, [one 1-D array per prompt]).
        `length` (seconds; None = the reference's fixed 10 s) may be one value or one per prompt: the clip is padded or cut to it, and each array
        comes back trimmed to min(its recording's length, its duration).  `conditioning_scale`, `surpass_noise`, `guidance_scale`,
        `guidance_rescale`, `eta` and `random_seed` may be lists with one entry per prompt; `ddim_steps` stays one value.  Every clip's energy curve
        is normalised by its own maximum, and every prompt comes out as the call with it alone gives it."""
        check_solver(solver, eta)
        sr = self.params['autoencoder']['sr']
        latent_sr = self.params['autoencoder']['latent_sr']
        batched = not isinstance(text, str)
        if isinstance(ddim_steps, (list, tuple)):
            raise ValueError('ddim_steps must be one value per call: per-prompt step counts are not supported')
        if batched != isinstance(audio_path, (list, tuple)) or (batched and len(audio_path) != len(text)):
            raise ValueError('a list of prompts needs a list of recordings of the same size (and the other way round)')
        for name, v in (('conditioning_scale', conditioning_scale), ('surpass_noise', surpass_noise), ('guidance_scale', guidance_scale),
                        ('guidance_rescale', guidance_rescale), ('eta', eta), ('random_seed', random_seed), ('length', length)):
            if isinstance(v, (list, tuple)) and (not batched or len(v) != len(text)):
                raise ValueError(f'a list of {name} needs a list of prompts of the same size')
        if not batched:
            seconds = 10 if length is None else length
            gt, original_length = self._load_clip(audio_path, surpass_noise, seconds)
            num_samples = len(gt)
            audio_frames = round(num_samples / sr * latent_sr) if length is None else int(round(length * latent_sr))
            gt_audio = torch.tensor(gt).unsqueeze(0).unsqueeze(1).to(self.device)
            latent_shape = (1, self.params['autoencoder']['dim'], audio_frames)   # the reference encodes only to get this shape
            condition = self.conditioner(gt_audio.squeeze(1), latent_shape)
            if length is not None:   # two control frames per latent frame, whatever the rounding of the duration left
                condition = torch.nn.functional.pad(condition, (0, max(0, 2 * audio_frames - condition.shape[-1])))[..., :2 * audio_frames]
            if randomize_seed:
                random_seed = random.randint(0, MAX_SEED)
            pred = inference_controlnet(self.autoencoder, self.unet, self.controlnet, None, None, condition, self.tokenizer,
                                        self.text_encoder, self.params, self.noise_scheduler, text, neg_text=None,
                                        audio_frames=audio_frames, guidance_scale=guidance_scale,
                                        guidance_rescale=guidance_rescale, ddim_steps=ddim_steps, eta=eta,
                                        random_seed=random_seed, conditioning_scale=conditioning_scale, device=self.device, solver=solver)
            pred = pred.cpu().numpy().squeeze(0).squeeze(0)[:original_length]
            return sr, pred
        n = len(text)
        seconds = list(length) if isinstance(length, (list, tuple)) else [10 if length is None else length] * n
        gates = list(surpass_noise) if isinstance(surpass_noise, (list, tuple)) else [surpass_noise] * n
        frames, conditions, keep = [], [], []
        for clip, gate, sec in zip(audio_path, gates, seconds):
            gt, original_length = self._load_clip(clip, gate, sec)
            f = int(round(sec * latent_sr))
            # per clip: the curve's normalisation takes THIS clip's maximum (a batch through the extractor would still do that per row, but clips differ in length)
            c = self.conditioner(torch.tensor(gt).unsqueeze(0).to(self.device), (1, self.params['autoencoder']['dim'], f))
            c = torch.nn.functional.pad(c, (0, max(0, 2 * f - c.shape[-1])))[..., :2 * f]
            frames.append(f)
            conditions.append(c)
            keep.append(min(original_length, len(gt)))
        if randomize_seed:
            random_seed = [random.randint(0, MAX_SEED) for _ in text]
        pred = inference_controlnet(self.autoencoder, self.unet, self.controlnet, None, None, conditions, self.tokenizer,
                                    self.text_encoder, self.params, self.noise_scheduler, list(text), neg_text=None,
                                    audio_frames=frames, guidance_scale=guidance_scale,
                                    guidance_rescale=guidance_rescale, ddim_steps=ddim_steps, eta=eta,
                                    random_seed=random_seed, conditioning_scale=conditioning_scale, device=self.device, solver=solver)
        pred = pred.cpu().numpy()
        return sr, [pred[i, 0, :k] for i, k in enumerate(keep)]
