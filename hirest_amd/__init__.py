"""hirest_amd — MI355X-native implementation of HiREST's frame/text encoding + cross-modal
scoring hot path.  Host side mirrors the reference's Python interface; all
compute is in libhirest_hip.so (include/hirest_hip.h)."""
from .eva_clip import (EVA_CLIP, build_eva_model_and_transforms, create_model, image_transform,  # noqa: F401
                       get_model_config, list_models)
from .tokenizer import tokenize  # noqa: F401
from .moment_model import MomentModel  # noqa: F401
from .sentence_encoder import SentenceTransformer  # noqa: F401
from .bert_score import BERTScorer  # noqa: F401
from .evaluation import evaluate_bert_score  # noqa: F401
from . import optim  # noqa: F401
from . import cascade  # noqa: F401
from . import whisper  # noqa: F401
from .cascade import run_end_to_end, end_to_end_results  # noqa: F401
# (the function takes the submodule's name in this namespace; its helpers: ``from hirest_amd.predict import merge_rank_results``)
from .predict import predict  # noqa: F401

__version__ = "0.1.0"
