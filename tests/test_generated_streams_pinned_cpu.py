"""The generated instruction streams are pinned: the nine .inc files csrc/Makefile builds from tools/gen_*.py, byte for byte.

The simulator tests (test_streams_cpu.py, test_dw_streams_cpu.py) check that a stream computes the right thing; this one checks that an
edit of a generator or of tools/mfma_stream.py that was MEANT to be neutral left every stream alone -- same text, same compile inputs,
same kernels.  A change that means to move a stream updates the hash here in the same commit and says why."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# product -> (generator, the Makefile's arguments with its default knob variables, sha256 of the product)
PINNED = {
    "sn_bf16_trunk.inc": ("gen_bf16_trunk.py", [], "0bee8c04fa53c195e28f799093bb283783aa8247f2a6fad15d178a4488767acb"),
    "sn_f16_trunk.inc": ("gen_bf16_trunk.py", ["f16=1"], "db1bd8d001bfe93cd498316a4c5fff8a8c6e81c844b4925b571b0ef835e69050"),
    "sn_bf16_trunk_t.inc": ("gen_bf16_trunk.py", ["store=1", "cap=6"], "4a6bcd7d80ba184749697a51b2ad94643a4609f33691aa71b46c0ea56c6095b6"),
    "sn_bf16_chain_t.inc": ("gen_bf16_chain.py", [], "57fc7c5171dec1135d2d64efd2f110b793fbfa5069ceed7ba662dd87c9543685"),
    "sn_x3_trunk.inc": ("gen_x3_trunk.py", [], "1782d0452a4fd359dc6b85270681710bba4010761a6dfcf74551f1c689cf06f0"),
    "sn_x3_chain.inc": ("gen_x3_chain.py", [], "a392b0e1d3bd98177ec5858b2497c1520ab9c6ec34a2fb05d4cfd3000208f66d"),
    "sn_dw_f32_chunk.inc": ("gen_dw_f32.py", [], "12030ce391130357a11a7625d9dcb76ad6d5e1e4ffc65b71afe1f51271d593db"),
    "sn_dw_bf16_chunk.inc": ("gen_dw_bf16.py", [], "815ae1a2fa59aaf2aaeec4df7ff10584aaa90059dafc8026330d4181d192dfb7"),
    "sn_dw_narrow_chunk.inc": ("gen_dw_narrow.py", [], "dd4630dbafd03024d8de3cad06433f2b1fe198de4e71d0144696462fbe3abf61"),
}


def test_generated_streams_are_pinned(tmp_path):
    got = {}
    for product, (tool, args, _) in PINNED.items():                  # the command lines of csrc/Makefile
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), str(tmp_path / product)] + args, check=True,
                       cwd=str(tmp_path), stdout=subprocess.DEVNULL)
        got[product] = hashlib.sha256((tmp_path / product).read_bytes()).hexdigest()
    assert got == {product: sha for product, (_, _, sha) in PINNED.items()}
