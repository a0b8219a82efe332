"""A CPU fp32 mode whose bits do not depend on the host: MKL's reproducibility branch COMPATIBLE, ATen's portable kernels (no
AVX2 / AVX-512 dispatch) and one intra-op thread. In the default mode the oracle's and the reference's logits carry the bits of
the CPU vendor, its vector width and the thread count, so a fixture recorded on one host is not bit-exact on another.

The LM fixtures (tests/golden/lm_*.npz) are recorded in this mode (oracle/make_golden.py) and tests/test_oracle_lm.py recomputes
them in it. The variables are read when torch starts: set them in the environment of a fresh process, before `import torch`."""

ENV = {"MKL_CBWR": "COMPATIBLE", "ATEN_CPU_CAPABILITY": "default"}
THREADS = 1
