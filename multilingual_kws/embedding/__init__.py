"""`multilingual_kws.embedding.<module>` = `multilingual_kws_amd.embedding.<module>` (the same module object): the drop-in modules under
the reference's own import path."""
import importlib
import sys

_MODULES = ("input_data", "transfer_learning", "batch_streaming_analysis", "single_target_recognize_commands", "distance_filtering", "tpr_fpr",
            "transfer_learning_analysis", "word_extraction", "generate_stream_sentences", "selection_eval")

for _m in _MODULES:
    _mod = importlib.import_module("multilingual_kws_amd.embedding." + _m)
    sys.modules[__name__ + "." + _m] = _mod
    globals()[_m] = _mod
del _m, _mod
