"""mpc-jellyfish_amd -- host-side mirror of the jf-plonk prover's arithmetic boundary on MI355X.

The package is a thin Python layer over libmi355zk.so (HIP, gfx950; C ABI in include/mzk.h):

    params   curve / field constants and host-side encodings (Python ints <-> Montgomery limbs)
    lib      ctypes binding of the C ABI; raises if the HIP library is missing (no CPU fallback)
    domain   Radix2EvaluationDomain mirror  (ark-poly surface used at prover.rs:54-62,545-567,672)
    kzg      UnivariateKzgPCS mirror        (primitives/src/pcs/univariate_kzg/mod.rs:90-377: commit, open, verify, their batches and multi_open_rou; srs.rs)
    plonk    TurboPlonk quotient round      (plonk/src/proof_system/prover.rs:512-759)
    sharding multi-GPU split of the commit path
    keys     ProvingKey / VerifyingKey as their ark-serialize images (structs.rs:575-590, 682-707), decoded on the GPU
    vid      Advz<E, Sha256> verifiable information dispersal (primitives/src/vid/advz.rs): disperse, verify, recover on the GPU

The directory name carries a hyphen, so import it with
    importlib.import_module("mpc-jellyfish_amd")      or      import mpc_jellyfish_amd   (shim at the repo root).
"""
from . import params  # noqa: F401
from .lib import MzkError, lib_path, load  # noqa: F401
from .domain import Radix2EvaluationDomain  # noqa: F401
from . import batch, linking, plonk, poly, prover, rng, sharding, snark, transcript  # noqa: F401
from .kzg import (Commitment, PCSError, SerializationError, UnivariateKzgPCS, UnivariateProverParam,  # noqa: F401
                  UnivariateUniversalParams, checked_fft_size, jacobian_to_affine, msm_bigint, msm_bigint_batch)
from . import keys  # noqa: F401
from . import vid  # noqa: F401
from .vid import Advz, VidError  # noqa: F401
from .keys import KeySerializationError, OpenKey, ProvingKey, VerifyingKey, key_layout  # noqa: F401
