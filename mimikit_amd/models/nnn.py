"""The concatenative generator: continue a prompt with the corpus frames that follow its best match.

Behaviour of the reference's ``NearestNextNeighbor`` (``mimikit/models/nnn.py:14-49``): the prompt's magnitude frames are aligned
against a corpus of frames by subsequence DTW over cosine distances (``librosa.sequence.dtw(C=pairwise_distances(|x|, |y|, 'cosine'),
subseq=True)``), the start frame is the column after the one where the best path ends, and every step returns the next corpus frame.

Here the alignment runs on the device for a whole batch at once (``csrc/nnn.hip``: the cost kernel reads the corpus once for all clips,
one wave per clip runs the DTW) - the reference takes every clip to the host (``x.detach().cpu().numpy()``).  Only the end column of the
path is computed: ``path[-1, -1]`` is ``argmin_j D[N-1, j]`` (first minimum), no back-pointers are needed.  Two deviations:

* the reference fails once a cursor reaches the end of the corpus (``snd[i:i+1]`` is empty); here the frame index is clamped to
  ``M - 1``, so the last frame repeats;
* prompts of more than ``native.NNN_MAX_ROWS`` frames raise ``NotImplementedError``.

NaN in the frames is not handled.
"""
from typing import Optional

import torch

from .. import native
from ..utils import default_device

__all__ = ["NearestNextNeighbor"]


class NearestNextNeighbor:
    def __init__(self, feature, snd: torch.Tensor, path_length: int = 16, sr: Optional[int] = None, device=None):
        snd = torch.as_tensor(snd)
        if snd.dim() != 1:
            raise ValueError(f"NearestNextNeighbor: snd must be a 1-D waveform, got shape {tuple(snd.shape)}")
        device = default_device() if device is None else device
        frames = feature(snd.to(device=device, dtype=torch.float32)[None])[0]
        self._bind(frames, feature, path_length, sr)

    @classmethod
    def from_frames(cls, frames: torch.Tensor, feature=None, sr: Optional[int] = None, path_length: int = 16) -> "NearestNextNeighbor":
        """bind a ready (M, bins) corpus of frames (on the device)"""
        self = cls.__new__(cls)
        self._bind(frames, feature, path_length, sr)
        return self

    def _bind(self, frames: torch.Tensor, feature, path_length: int, sr: Optional[int]):
        if not isinstance(frames, torch.Tensor) or frames.dim() != 2 or frames.shape[0] < 1 or frames.shape[1] < 1:
            raise ValueError(f"NearestNextNeighbor: the corpus must be (M >= 1, bins >= 1) frames, got {tuple(getattr(frames, 'shape', ()))}")
        self.feature = feature
        self.sr = sr
        self.snd = frames.float().contiguous()           # (the reference's name for the corpus frames)
        # the inverse norms are computed once, where the corpus reaches the device (a corpus bound on the host is only held: `to`)
        self.snd_inv_norm = native.inv_row_norm(self.snd) if self.snd.is_cuda else None
        self.shift = path_length                         # stored as the reference stores it; the alignment does not use it (nor does the reference's)
        self._t = -100
        self._starts = None

    # -- the ARM-like surface the ensemble needs ------------------------------------------------------
    @property
    def device(self):
        return self.snd.device

    def to(self, device):
        snd = self.snd.to(device)
        if snd is not self.snd:
            self.snd, self.snd_inv_norm, self._starts = snd, None, None
        if self.snd_inv_norm is None and self.snd.is_cuda:
            self.snd_inv_norm = native.inv_row_norm(self.snd)
        return self

    @property
    def n_frames(self) -> int:
        return self.snd.shape[0]

    @property
    def n_bins(self) -> int:
        return self.snd.shape[1]

    # -- alignment ------------------------------------------------------------------------------------
    def predict_start_frames(self, X: torch.Tensor) -> torch.Tensor:
        """X: (B, N, bins) prompt frames -> int64 (B,) on the device: the corpus frame after the one where each clip's best alignment ends"""
        if X.dim() == 2:
            X = X[None]
        if X.dim() != 3:
            raise ValueError(f"NearestNextNeighbor: prompt frames must be (B, N, bins), got {tuple(X.shape)}")
        if X.shape[1] > native.NNN_MAX_ROWS:
            raise NotImplementedError(f"NearestNextNeighbor: N = {X.shape[1]} prompt frames, the device alignment takes at most "
                                      f"{native.NNN_MAX_ROWS} (one wave per clip)")
        if X.shape[2] != self.n_bins:
            raise ValueError(f"NearestNextNeighbor: the prompt has {X.shape[2]} bins, the corpus {self.n_bins}")
        native.require_device(X, self.snd)
        end, _ = native.nnn_end_columns(X if X.dtype == torch.float32 else X.float(), self.snd, self.snd_inv_norm)
        return end + 1

    def predict_start_frame(self, X: torch.Tensor) -> torch.Tensor:
        """one clip's (N, bins) -> 0-d int64 tensor (the reference's method; stays on the device)"""
        return self.predict_start_frames(X[None])[0]

    @staticmethod
    def _prompt(inputs) -> torch.Tensor:
        return inputs[0] if isinstance(inputs, (tuple, list)) else inputs

    def _rows(self, index: torch.Tensor) -> torch.Tensor:
        return self.snd[index.clamp(max=self.n_frames - 1)]

    def generate_step(self, t: int, inputs, ctx=None) -> torch.Tensor:
        """re-align when ``t`` does not follow the last call's, then return the corpus frame at each clip's cursor, (B, 1, bins), and advance"""
        if t != self._t + 1 or self._starts is None:
            self._starts = self.predict_start_frames(self._prompt(inputs))
            self._t = t - 1
        out = self._rows(self._starts)[:, None]
        self._starts = self._starts + 1
        self._t += 1
        return out

    def generate_block(self, inputs, n_steps: int) -> torch.Tensor:
        """``n_steps`` consecutive ``generate_step`` outputs after a fresh alignment as one gather: (B, n_steps, bins)"""
        starts = self.predict_start_frames(self._prompt(inputs))
        index = starts[:, None] + torch.arange(n_steps, device=starts.device)
        return self._rows(index)
