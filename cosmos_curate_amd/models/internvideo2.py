"""InternVideo2MultiModality ModelInterface — the video embedder.

Counterpart of the reference's models/internvideo2_mm.py
``InternVideo2MultiModality``, vision side only: ``get_target_num_frames``,
``formulate_input_frames`` (delegates to internvideo2_prep, the bit-exact
device mirror of the reference's frame construction) and
``encode_batched_videos`` on the MFMA tower
(internvideo2_vit.InternVideo2VisionTowerAMD).  The text tower
(``get_text_embedding`` / ``evaluate``) is not implemented and says so.

Weights: ``checkpoint_path`` (or ``CC_IV2_CHECKPOINT``) names a local
InternVideo2 stage-2 ``.pth``; without one the deterministic stand-in
weights are used (internvideo2_weights).  A checkpoint whose position table
is for another number of frames than ``num_frames`` raises at setup().
"""

from __future__ import annotations

import dataclasses
import os

import numpy as np
import numpy.typing as npt
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.core.interfaces.model_interface import ModelInterface
from cosmos_curate_amd.models import internvideo2_prep as prep
from cosmos_curate_amd.models import internvideo2_weights as iw

_INTERNVIDEO2_MODEL_ID = "OpenGVLab/InternVideo2-Stage2_1B-224p-f4"


class InternVideo2MultiModality(ModelInterface):
    """``utils_only``: frame preparation only, no tower (the frame-creation
    stage's instance).  ``tower``: a ready tower to use instead of building
    one (tests inject a 2-block tower)."""

    def __init__(
        self,
        *,
        utils_only: bool = False,
        num_frames: int = iw.INTERNVIDEO2_1B.num_frames,
        checkpoint_path: str | None = None,
        tower: torch.nn.Module | None = None,
    ) -> None:
        super().__init__()
        self.utils_only = utils_only
        self._cfg = (tower.cfg if tower is not None else
                     dataclasses.replace(iw.INTERNVIDEO2_1B, num_frames=num_frames))
        self._checkpoint_path = checkpoint_path
        self._tower = tower

    @property
    def conda_env_name(self) -> str:
        return "unified"

    @property
    def model_id_names(self) -> list[str]:
        return [_INTERNVIDEO2_MODEL_ID]

    def setup(self) -> None:
        if self.utils_only or self._tower is not None:
            return
        from cosmos_curate_amd.models.internvideo2_vit import InternVideo2VisionTowerAMD

        hotpath.require_gpu()  # fail loudly before any lazy surprises
        path = self._checkpoint_path or os.environ.get("CC_IV2_CHECKPOINT")
        sd = (iw.load_internvideo2_state_dict(path) if path
              else iw.make_internvideo2_weights(self._cfg))
        self._tower = InternVideo2VisionTowerAMD(sd, self._cfg).to("cuda")

    def get_target_num_frames(self) -> int:
        return self._cfg.num_frames

    def formulate_input_frames(self, frames: torch.Tensor | npt.NDArray[np.uint8]) -> torch.Tensor:
        """(N, H, W, 3) u8 frames -> (1, T, 3, image, image) f32 on the
        device; an empty tensor when there are fewer than T frames (the
        reference returns an empty array there)."""
        hotpath.require_gpu()
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        frames = frames.to("cuda")
        if frames.shape[0] < self._cfg.num_frames:
            return torch.empty(0, dtype=torch.float32, device=frames.device)
        return prep.formulate_input_frames(
            frames, fnum=self._cfg.num_frames, target_size=self._cfg.image)

    def _patches_u8(self, frames_u8: torch.Tensor) -> torch.Tensor:
        """(N, image, image, 3) u8 device frames -> the patch GEMM's A rows,
        normalised with the InternVideo2 mean / std in the same kernel."""
        import ctypes

        lib = hotpath.require_gpu()
        cfg = self._cfg
        n, h, w, _ = frames_u8.shape
        patch_k = self._tower.patch_k
        out = torch.empty((n * cfg.tokens_per_frame, patch_k),
                          dtype=torch.bfloat16, device=frames_u8.device)
        stream = torch.cuda.current_stream(frames_u8.device).cuda_stream
        mean = (ctypes.c_float * 3)(*prep.IV2_MEAN)
        std = (ctypes.c_float * 3)(*prep.IV2_STD)
        hotpath.check(lib.cc_clip_preprocess_patches(
            frames_u8.contiguous().data_ptr(), n, h, w, cfg.patch, patch_k,
            mean, std, out.data_ptr(), stream))
        return out

    @torch.no_grad()
    def encode_batched_videos(
        self, videos: torch.Tensor | list[torch.Tensor], batch_size: int = 8,
    ) -> torch.Tensor:
        """(B, T, image, image, 3) u8 device frames, the prepared
        (B, T, 3, image, image) float tensor, or a list of per-clip
        (1, T, 3, image, image) tensors as formulate_input_frames returns
        them -> (B, proj) f32 unit-norm, at most ``batch_size`` clips per
        forward."""
        assert self._tower is not None, "setup() not called"
        if isinstance(videos, (list, tuple)):
            videos = torch.cat(list(videos), dim=0)
        cfg = self._cfg
        videos = videos.to("cuda")
        outs = []
        for i in range(0, videos.shape[0], batch_size):
            chunk = videos[i : i + batch_size]
            if chunk.dtype == torch.uint8:
                want = (cfg.num_frames, cfg.image, cfg.image, 3)
                if tuple(chunk.shape[1:]) != want:
                    msg = f"expected (B, {want}) u8 frames, got {tuple(chunk.shape)}"
                    raise ValueError(msg)
                outs.append(self._tower(
                    patches=self._patches_u8(chunk.flatten(0, 1)), n=chunk.shape[0]))
            else:
                outs.append(self._tower(chunk))
        return torch.cat(outs, dim=0)

    def get_text_embedding(self, text: str) -> torch.Tensor:
        msg = "the InternVideo2 text tower is not implemented"
        raise NotImplementedError(msg)

    def evaluate(self, video_embd: torch.Tensor, text_embds: list[torch.Tensor]):
        msg = "the InternVideo2 text tower is not implemented"
        raise NotImplementedError(msg)
