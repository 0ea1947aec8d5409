"""Attack plugin API of the hot path (reference: adversarial_attacks/torchattacks/__init__.py).

The attacks the north-star path names — FGSM, PGD, PGDL2, CW — FAB (the attack that completes the
reference's AttackEnum), APGD (the step-size-free gradient attack of AutoAttack), APGDL1 (its L1 member) and the momentum attacks made for
transfer between detectors (MI-FGSM, NI-FGSM and their variance-tuned forms), MultiAttack (the worst case over a list
of them), MinRadiusPGD (each utterance's minimal radius, by bisection on the device), PGDSNR (PGD under a budget in dB of
SNR or segmental SNR), UniversalPGD (one perturbation fitted once and added to every utterance) and SPSA (the score-based
black-box counterpart of PGD: queries instead of gradients) and EOTPGD (PGD on a gradient summed over passes, here over draws of a
simulated audio channel: `Channel`, `CHANNELS`) and PGDL0 (the sparse threat model: at most k samples of an utterance change) and HopSkipJump (the label-only
black-box attack: decisions instead of scores) and PsyPGD (PGD pulled under the psychoacoustic masking threshold of the clean
utterance: `MaskingModel`), and beside them `Smoothing`, which is no attack: randomized smoothing's votes over noisy copies, for a
certified lower bound on the radius the attacks bound from above, and SmoothAdvPGD (PGD on that smoothed detector's soft vote: the
adversary the certificate has to withstand) and FMN (the minimal-norm attack: every utterance's radius in one run, without a
largest radius and without an outer search) and FMNSparse (its L1 and L0 forms: the minimal L1 norm and the minimal number of
changed samples) and UniversalFilter (the convolutive threat model: one short FIR filter fitted once and applied to every fake,
after Malafide), with the reference's constructor
signatures and the reference's 1-logit -> 2-logit adapter (`cat([-z, z], 1)`)."""
from .attack import Attack
from .attacks.apgd import APGD
from .attacks.apgdl1 import APGDL1
from .attacks.cw import CW
from .attacks.eotpgd import EOTPGD
from .attacks.fab import FAB
from .attacks.fgsm import FGSM
from .attacks.filter import UniversalFilter
from .attacks.fmn import FMN
from .attacks.fmn_sparse import FMNSparse
from .attacks.hopskipjump import HopSkipJump
from .attacks.mifgsm import MIFGSM
from .attacks.minradius import MinRadiusPGD
from .attacks.multiattack import MultiAttack
from .attacks.nifgsm import NIFGSM
from .attacks.pgd import PGD
from .attacks.pgdl0 import PGDL0
from .attacks.pgdl2 import PGDL2
from .attacks.pgdsnr import PGDSNR
from .attacks.psypgd import PsyPGD
from .attacks.smoothadv import SmoothAdvPGD
from .attacks.spsa import SPSA
from .attacks.universal import UniversalPGD
from .attacks.vmifgsm import VMIFGSM
from .attacks.vnifgsm import VNIFGSM
from .channel import CHANNELS, Channel
from .masking import MaskingModel
from .smoothing import Smoothing

__version__ = "3.2.7+advstep"
__all__ = ["Attack", "FGSM", "PGD", "PGDL2", "CW", "FAB", "APGD", "APGDL1", "MIFGSM", "NIFGSM", "VMIFGSM", "VNIFGSM",
           "MultiAttack", "MinRadiusPGD", "PGDSNR", "UniversalPGD", "SPSA", "EOTPGD", "Channel", "CHANNELS",
           "PGDL0", "HopSkipJump", "PsyPGD", "MaskingModel", "Smoothing", "SmoothAdvPGD", "FMN",
           "FMNSparse", "UniversalFilter"]
