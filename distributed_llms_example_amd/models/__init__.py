"""Encoder-decoder model families on the fused-op library: T5 / mT5 / FLAN-T5 / LongT5-local (models/t5.py) and BART /
mBART / Pegasus / Marian / M2M100-NLLB / PLBart /
Blenderbot / LED (models/bart.py), and T5Gemma (models/t5gemma.py)."""
from .bart import BartForConditionalGeneration
from .config import PRESETS, Seq2SeqConfig, resolve_config
from .distill import Distill, make_student
from .preference import Preference
from .hf_io import build_model, from_hf_state_dict, from_pretrained, save_pretrained, to_hf_state_dict
from .t5 import T5ForConditionalGeneration
from .t5gemma import T5GemmaForConditionalGeneration

__all__ = ["PRESETS", "Seq2SeqConfig", "resolve_config", "build_model", "from_pretrained", "save_pretrained",
           "to_hf_state_dict", "from_hf_state_dict", "T5ForConditionalGeneration", "BartForConditionalGeneration",
           "T5GemmaForConditionalGeneration", "Distill", "make_student", "Preference"]
