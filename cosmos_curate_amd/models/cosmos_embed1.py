"""CosmosEmbed1 ModelInterface — the ``cosmos-embed1-*`` video embedder.

Counterpart of the reference's models/cosmos_embed1.py ``CosmosEmbed1``,
vision side only: ``get_target_num_frames``, ``formulate_input_frames`` (the
IV2 subsample rule ``[::len//T][:T]`` and the device resize + normalise of
internvideo2_prep at the variant's resolution, with the config's mean / std)
and ``encode_video_frames`` on the MFMA tower
(cosmos_embed1_vit.CosmosEmbed1TowerAMD).  The text tower
(``get_text_embedding`` / ``evaluate``) is not implemented and says so.

Weights: the deterministic stand-ins (cosmos_embed1_vit); mapping the
published checkpoint's names onto the tower's is not implemented.
"""

from __future__ import annotations

import numpy as np
import numpy.typing as npt
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.core.interfaces.model_interface import ModelInterface
from cosmos_curate_amd.models import cosmos_embed1_vit as cv
from cosmos_curate_amd.models import internvideo2_prep as prep


class CosmosEmbed1(ModelInterface):
    """``utils_only``: frame preparation only, no tower (the frame-creation
    stage's instance).  ``tower``: a ready tower to use instead of building
    one (tests inject a reduced-depth tower)."""

    def __init__(
        self,
        *,
        variant: str = "336p",
        utils_only: bool = False,
        tower: torch.nn.Module | None = None,
    ) -> None:
        super().__init__()
        if variant not in cv.VARIANTS:
            raise ValueError(
                f"variant must be one of {sorted(cv.VARIANTS)}, got {variant!r}")
        self.variant = variant
        self.utils_only = utils_only
        self._cfg = tower.cfg if tower is not None else cv.VARIANTS[variant]
        self._tower = tower

    @property
    def conda_env_name(self) -> str:
        return "unified"

    @property
    def model_id_names(self) -> list[str]:
        return [f"nvidia/Cosmos-Embed1-{self.variant}"]

    def setup(self) -> None:
        if self.utils_only or self._tower is not None:
            return
        hotpath.require_gpu()  # fail loudly before any lazy surprises
        self._tower = cv.CosmosEmbed1TowerAMD(
            cv.make_cosmos_embed1_weights(self._cfg), self._cfg).to("cuda")

    def get_target_num_frames(self) -> int:
        return self._cfg.num_frames

    def formulate_input_frames(
        self, frames: torch.Tensor | npt.NDArray[np.uint8]
    ) -> torch.Tensor:
        """(N, H, W, 3) u8 frames -> (1, T, 3, image, image) f32 on the
        device; an empty tensor when there are fewer than T frames."""
        hotpath.require_gpu()
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        frames = frames.to("cuda")
        cfg = self._cfg
        if frames.shape[0] < cfg.num_frames:
            return torch.empty(0, dtype=torch.float32, device=frames.device)
        return prep.formulate_input_frames(
            frames, fnum=cfg.num_frames, target_size=cfg.image, mean=cfg.mean,
            std=cfg.std)

    @torch.no_grad()
    def encode_video_frames(
        self, frames: torch.Tensor | list[torch.Tensor], batch_size: int = 8,
    ) -> torch.Tensor:
        """The prepared (B, T, 3, image, image) float tensor, or a list of
        per-clip (1, T, 3, image, image) tensors as formulate_input_frames
        returns them -> (B, D) f32 unit-norm, at most ``batch_size`` clips
        per forward."""
        assert self._tower is not None, "setup() not called"
        if isinstance(frames, (list, tuple)):
            frames = torch.cat(list(frames), dim=0)
        frames = frames.to("cuda")
        if frames.numel() == 0:
            return torch.empty((0, self._cfg.proj), dtype=torch.float32)
        return torch.cat([self._tower(frames[i : i + batch_size])
                          for i in range(0, frames.shape[0], batch_size)], dim=0)

    def get_text_embedding(self, text: str) -> torch.Tensor:
        msg = "the Cosmos-Embed1 text tower is not implemented"
        raise NotImplementedError(msg)

    def evaluate(self, video_embd: torch.Tensor, text_embds: list[torch.Tensor]):
        msg = "the Cosmos-Embed1 text tower is not implemented"
        raise NotImplementedError(msg)
