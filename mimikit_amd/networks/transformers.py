"""SimpleTransformer behind the ARM protocol, generating on the MI355X.

Config fields, module wiring and ``state_dict`` layout follow the reference (``mimikit/networks/transformers.py``:
``PositionalEncoding`` :23-67, ``SimpleTransformer`` :70-178): the decoder is a stock ``nn.TransformerDecoder`` that holds the
weights, so reference checkpoints load unchanged.

Generation is the reference's arithmetic: every step re-embeds the rf-long window, adds ``pe[0:rf]`` and runs all decoder layers
(causal self-attention, causal cross-attention with ``memory = src``) over it, then keeps the last position.  ``eval()`` forward,
``generate_step`` and ``generate_block`` run only on the HIP device (``csrc/transformer_plan.hip``); training-mode ``forward`` is
the stock differentiable torch graph.  Covered IO: ``IOSpec.mulaw_io(input_module_type="embedding")`` (embedding in, MLP head +
CategoricalSampler out) and ``IOSpec.magspec_io`` (Linear in, Linear + Abs out); DESIGN.md section 5.8.
"""
import dataclasses as dtc
import math
from typing import Set, Tuple

import torch
import torch.nn as nn
from torch.nn import TransformerDecoder, TransformerDecoderLayer

from .. import native
from ..features.item_spec import ItemSpec, Step
from ..io_spec import IOSpec
from ..modules.io import ZipReduceVariables
from ..modules.misc import Chunk
from ..modules.targets import OutputWrapper
from .arm import ARM, NetworkConfig
from .hip_plan import HipPlanned, describe_head

__all__ = ["PositionalEncoding", "SimpleTransformer"]


class PositionalEncoding(nn.Module):
    """sin / cos absolute positions (transformers.py:23-67); the table is the buffer ``pe`` of shape (max_len, 1, d_model)"""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        pe = pe.unsqueeze(0).transpose(0, 1)
        self.register_buffer('pe', pe)

    def forward(self, x):
        x = x + self.pe[:x.size(0), :]
        return self.dropout(x)


class SimpleTransformer(HipPlanned, ARM, nn.Module):
    @dtc.dataclass
    class Config(NetworkConfig):
        io_spec: IOSpec = None
        model_dim: int = 256
        n_heads: int = 8
        feedforward_dim: int = 1024
        num_layers: int = 8
        with_layer_norm: bool = False
        dropout: float = 0.0
        input_dropout: float = .1
        rf: int = 64

    @classmethod
    def from_config(cls, config: "SimpleTransformer.Config"):
        layer = TransformerDecoderLayer(d_model=config.model_dim, nhead=config.n_heads, dim_feedforward=config.feedforward_dim,
                                        dropout=config.dropout, activation="relu")
        model = TransformerDecoder(layer, num_layers=config.num_layers,
                                   norm=None if not config.with_layer_norm else nn.LayerNorm(config.model_dim))
        input_modules = [spec.module.copy().set(out_dim=config.model_dim).module() for spec in config.io_spec.inputs]
        input_module = ZipReduceVariables(mode="sum", modules=input_modules)
        output_modules = [spec.module.copy().set(in_dim=config.model_dim).module() for spec in config.io_spec.targets]
        return cls(config, model, input_module=input_module, output_modules=output_modules)

    def __init__(self, config: "SimpleTransformer.Config", transformer, input_module, output_modules):
        super().__init__()
        self._config = config
        self.model = transformer
        self.input_module = input_module
        self.output_modules = nn.ModuleList(output_modules)
        self.dp1d = nn.Dropout1d(config.input_dropout)
        self.src_mask = None
        self.tgt_padding_mask = None
        self.pe = PositionalEncoding(config.model_dim, dropout=0., max_len=2048)

    # -- ARM properties -----------------------------------------------------------
    @property
    def config(self) -> NetworkConfig:
        return self._config

    @property
    def rf(self):
        return self._config.rf

    @property
    def generate_params(self) -> Set[str]:
        return {"temperature"}

    def train_batch(self, item_spec: ItemSpec):
        return tuple(
            spec.to_batch_item(item_spec) for spec in self.config.io_spec.inputs
        ), tuple(
            spec.to_batch_item(ItemSpec(shift=1, length=0, unit=Step()) + item_spec) for spec in self.config.io_spec.targets
        )

    def test_batch(self, item_spec: ItemSpec):
        return self.train_batch(item_spec)

    # -- forward ------------------------------------------------------------------------
    def _generate_square_subsequent_mask(self, sz):
        mask = (torch.triu(torch.ones(sz, sz)) == 1).transpose(0, 1)
        return mask.float().masked_fill(mask == 0, float('-inf')).masked_fill(mask == 1, float(0.0))

    def _forward_autograd(self, src: Tuple, **parameters):
        src = self.input_module(src)
        if self.training:
            src = self.dp1d(src)
        src = src.permute(1, 0, 2).contiguous()
        src = self.pe(src)
        if self.src_mask is None or self.src_mask.size(0) != len(src):
            self.src_mask = self._generate_square_subsequent_mask(len(src)).to(src.device)
            self.tgt_padding_mask = torch.zeros(src.size(1), len(src), dtype=torch.bool, device=src.device)
            self.tgt_padding_mask[0] = True
        out = self.model(tgt=src, memory=src, tgt_mask=self.src_mask, memory_mask=self.src_mask).permute(1, 0, 2).contiguous()
        if not self.training:
            out = out[:, -1:]
        return tuple(mod(out, **parameters) for mod in self.output_modules)

    def forward(self, src: Tuple, **parameters):
        if self.training:
            return self._forward_autograd(src, **parameters)
        return self._device_step(tuple(src), **parameters)

    # -- HIP plan (the lifecycle: hip_plan.HipPlanned) ---------------------------------
    _plan_class = native.TransformerPlan
    _weights_checked_every_call = True

    def _describe(self, max_batch: int) -> native.TransformerConfig:
        cfg = self._config
        unsupported = []
        c = native.TransformerConfig()
        heads_in = list(self.input_module.heads)
        if len(heads_in) != 1 or len(self.output_modules) != 1:
            unsupported.append(f"{len(heads_in)} inputs and {len(self.output_modules)} targets (one of each is covered)")
        else:
            first = heads_in[0]
            core = first[0] if isinstance(first, nn.Sequential) else first
            tail = [m for m in list(first)[1:] if not (isinstance(m, Chunk) and m.chunks == 1)] if isinstance(first, nn.Sequential) else []
            if isinstance(core, nn.Embedding) and not tail and core.padding_idx is None and core.max_norm is None:
                c.in_kind, c.in_classes = 0, core.num_embeddings
            elif isinstance(core, nn.Linear) and core.bias is not None and not tail and core.out_features == cfg.model_dim:
                c.in_kind, c.in_dim = 1, core.in_features
            else:
                unsupported.append(f"input module {type(core).__name__} (EmbeddingIO or ChunkedLinearIO are covered)")
            sampled = isinstance(self.output_modules[0], OutputWrapper)
            kind, head, problem = describe_head(self.output_modules[0], self.training, need_sampler=True)
            if sampled and kind != "mlp":
                unsupported.append("output module other than MLPIO + CategoricalSampler")
            elif not sampled and (kind != "linear" or problem):
                unsupported.append("output module other than (Chunked)LinearIO [+ Abs]")
            elif problem:
                unsupported.append(problem)
            else:
                c.head_kind = int(kind == "linear")
                for name, value in head.items():
                    setattr(c, name, value)
            if not unsupported and (c.in_kind == 0) != (c.head_kind == 0):
                unsupported.append("class indices in with frames out, or frames in with class indices out")
        if unsupported:
            raise NotImplementedError("the HIP generate path does not cover: " + "; ".join(unsupported))
        c.model_dim, c.n_heads, c.feedforward_dim, c.num_layers, c.rf = cfg.model_dim, cfg.n_heads, cfg.feedforward_dim, cfg.num_layers, cfg.rf
        c.final_norm = int(self.model.norm is not None)
        c.max_batch = max_batch
        c.tuning = native.tuning_text(native.PLAN_TUNING, self.exec_tuning)
        return c

    def _check_temperature(self, temperature):
        if temperature is not None and not isinstance(self.output_modules[0], OutputWrapper):
            # the reference hands the temperature to the head's Sequential (transformers.py:178), which takes no keyword
            raise TypeError("Sequential.forward() got an unexpected keyword argument 'temperature'")

    def _prepare(self, x: torch.Tensor) -> torch.Tensor:
        if self._plan.cfg.in_kind == 0:
            x = x if x.dtype == torch.int64 else x.long()
            return x if x.stride(-1) == 1 else x.contiguous()
        x = x if x.dtype == torch.float32 else x.float()
        return x if x.stride(-1) == 1 else x.contiguous()

    def _device_step(self, inputs: Tuple[torch.Tensor, ...], temperature=None):
        if len(inputs) != 1:
            raise NotImplementedError(f"the HIP generate path does not cover: {len(inputs)} inputs (one is covered)")
        x = inputs[0]
        rf = self._config.rf
        if x.size(1) < rf:
            raise ValueError(f"a window of {x.size(1)} positions is shorter than rf={rf}: the reference's window slice is empty")
        if x.size(1) != rf:
            raise NotImplementedError(f"the HIP generate path does not cover: a window of {x.size(1)} positions (rf={rf} is covered)")
        self._check_temperature(temperature)
        native.require_device(*inputs)
        self._ensure_plan(x.size(0), refresh_weights=False)
        x = self._prepare(x)
        t, u = self._sampling(x.size(0), 1, temperature)
        y = self._plan.step(x, t, u)
        return (y.unsqueeze(1),)

    # -- ARM generation protocol ------------------------------------------------------
    def before_generate(self, prompts: Tuple[torch.Tensor, ...], batch_index) -> None:
        """the weights are checked; the plan's KV rows, step counter and stored graph need no reset: a call rewrites what it reads, and the
        graph is keyed by the call's pointers and strides (tests/test_gpu_plan_lives.py::test_transformer_plan_lives holds that)"""
        prompts = tuple(prompts)
        native.require_device(*prompts)
        self._ensure_plan(prompts[0].size(0), refresh_weights=True)

    def generate_step(self, inputs: Tuple[torch.Tensor, ...], *, t: int = 0, **parameters):
        return self._device_step(tuple(inputs), **parameters)

    def generate_block(self, tensors: Tuple[torch.Tensor, ...], t0: int, n_steps: int, **parameters):
        """all steps of one batch in one device call; the outputs are written in place into ``tensors[0]``"""
        tensors = tuple(tensors)
        if len(tensors) != 1:
            raise NotImplementedError(f"the HIP generate path does not cover: {len(tensors)} inputs (one is covered)")
        if t0 < self.rf:
            raise ValueError(f"a prompt of {t0} steps is shorter than rf={self.rf}: the reference's window slice is empty")
        self._check_temperature(parameters.get("temperature", None))
        native.require_device(*tensors)
        data = tensors[0]
        self._ensure_plan(data.size(0), refresh_weights=False)
        if self._prepare(data).data_ptr() != data.data_ptr():
            raise TypeError("generate_block writes in place: tensors[0] must be int64 classes / fp32 frames with unit stride on the last dim")
        t, u = self._sampling(data.size(0), n_steps, parameters.get("temperature", None))
        self._plan.generate(data, t0, n_steps, t, u)
        return True

    def after_generate(self, final_outputs: Tuple[torch.Tensor, ...], batch_index) -> None:
        pass
