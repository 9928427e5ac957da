"""mimi_hip — MI355X-native Mimi encode engine (drop-in for the potsawee/tokenize-audio encode path).

    from mimi_hip import MimiEncoder                 # replaces the scripts' `class MimiEncoder`
    from mimi_hip import MimiHipModel                # replaces transformers.MimiModel for .encode
    from mimi_hip import codes_to_chars              # replaces utils.codes_to_chars
    from mimi_hip import audio_to_str, str_to_audio  # replace utils.audio_to_str / utils.str_to_audio (decode=True)
    from mimi_hip import strs_to_audio               # a list of strings in ragged batches, each str_to_audio's bits

torch is imported lazily by the model modules; ``mimi_hip.config`` / ``mimi_hip.synthetic`` / ``mimi_hip.codes``
need only numpy.
"""
from .config import MimiConfig, encoded_length  # noqa: F401

__all__ = ["MimiConfig", "encoded_length", "MimiHipModel", "MimiEncoderOutput", "MimiDecoderOutput",
           "MimiEncoder", "MimiFeatureExtractor", "codes_to_chars", "chars_to_codes", "audio_to_str", "str_to_audio",
           "strs_to_audio"]


def __getattr__(name):
    if name in ("MimiHipModel", "MimiEncoderOutput", "MimiDecoderOutput"):
        from . import model
        return getattr(model, name)
    if name == "MimiEncoder":
        from .encoder import MimiEncoder
        return MimiEncoder
    if name == "MimiFeatureExtractor":
        from .feature_extraction import MimiFeatureExtractor
        return MimiFeatureExtractor
    if name in ("codes_to_chars", "chars_to_codes", "audio_to_str", "str_to_audio", "strs_to_audio"):
        from . import codes
        return getattr(codes, name)
    raise AttributeError(name)
