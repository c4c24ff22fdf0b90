"""Regenerates tests/golden/embed_launch_sequences.json on an MI355X (256 CUs, pair probe passed): the (stage, kernel) sequence of one
forward pass for the default-option handle classes, as tests/test_embedding_gpu.py::test_default_launch_sequences collects it.  Run it on
the commit whose plan is to be kept, BEFORE a change that is meant to leave the plan alone; an optional argument names another output file."""
import json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import torch                                                        # noqa: E402
import test_embedding_gpu as T                                      # noqa: E402
from multilingual_kws_amd import weights                            # noqa: E402
from multilingual_kws_amd.embedding_model import EmbeddingModel     # noqa: E402

blob = weights.synthetic_blob()
big = EmbeddingModel(blob, max_batch=1024)
assert torch.cuda.get_device_properties(0).multi_processor_count == 256 and big.get_option("fuse_pair") == 1
seqs = T._default_launch_sequences(blob, big, torch.device("cuda:0"))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "embed_launch_sequences.json")
json.dump(seqs, open(out, "w"), indent=0)
print({k: len(v) for k, v in seqs.items()})
