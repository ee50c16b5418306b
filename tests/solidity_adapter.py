"""Test side: the oracle's SolidityTranscript (oracle/pyref_fs.py:281-296) behind the PlonkTranscript interface that pyref_verifier,
pyref_snark and pyref_linking take from their caller.  Shared by the tests of the Keccak-256 transcript."""
import pyref_fs as FS

SOLIDITY = 4                                                       # MZK_TRANSCRIPT_SOLIDITY
CH = ("tau", "beta", "gamma", "alpha", "zeta", "v", "u")


class SolidityPlonkTranscript(FS.StandardTranscript):
    """the default append_* of PlonkTranscript over the oracle's SolidityTranscript; .lens: the transcript length at every challenge"""

    def __init__(self, c, label=b"PlonkProof"):
        self.c, self.s, self.lens = c, FS.SolidityTranscript(c), []

    def append_message(self, l, m):
        self.s.append_message(l, m)

    def append_field_elem(self, l, x):
        self.s.append_message(l, FS.fr_bytes(self.c, x))

    def append_commitment(self, l, p):
        self.s.append_message(l, FS.g1_bytes(self.c, p))

    def get_and_append_challenge(self, l):
        self.lens.append(len(self.s.buf))
        return self.s.get_and_append_challenge(l)


def oracle_batch_challenge(pc, us):
    """verifier.rs:203-215 under T = SolidityTranscript: r from the challenges u of K proofs (1 for one proof)"""
    if len(us) == 1:
        return 1
    t = SolidityPlonkTranscript(pc, b"batch verify")
    for u in us:
        t.append_field_elem(b"u", u)
    return t.get_and_append_challenge(b"r")
