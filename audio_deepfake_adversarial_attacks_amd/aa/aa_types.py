"""Attack registry: CLI name -> (attack class, kwargs)  (reference: src/aa/aa_types.py:5-24).

The reference's members are kept verbatim, FAB included.
Additive members carry the configurations BASELINE.json names, which the reference's enum cannot express
(SURVEY.md F7): 40-step PGD at eps = 0.003, 40-step PGDL2, and CW."""
from enum import Enum

from .. import torchattacks


def _worst_case_linf(eps, steps=10, apgd_steps=None):
    """The members of a WORSTCASE* entry within one L-inf radius, cheapest first, with the hyper-parameters of the single-attack
    members of the same radius below (alpha = eps / steps for MI-FGSM)."""
    return {"members": [("PGD", {"eps": eps, "steps": steps}),
                        ("MIFGSM", {"eps": eps, "alpha": eps / steps, "steps": steps, "decay": 1.0}),
                        ("APGD", {"norm": "Linf", "eps": eps, "steps": apgd_steps or steps})]}


class AttackEnum(Enum):

    # --- reference members (aa_types.py:8-22) ---
    PGD = (torchattacks.PGD, {"eps": 0.0005, "steps": 10})
    PGD_eps00075 = (torchattacks.PGD, {"eps": 0.00075, "steps": 10})
    PGD_eps001 = (torchattacks.PGD, {"eps": 0.001, "steps": 10})

    PGDL2 = (torchattacks.PGDL2, {"eps": 0.1, "steps": 10})
    PGDL2_eps15 = (torchattacks.PGDL2, {"eps": 0.15, "steps": 10})
    PGDL2_eps20 = (torchattacks.PGDL2, {"eps": 0.20, "steps": 10})

    FGSM = (torchattacks.FGSM, {"eps": 0.0005})
    FGSM_eps00075 = (torchattacks.FGSM, {"eps": 0.00075})
    FGSM_eps001 = (torchattacks.FGSM, {"eps": 0.001})

    FAB = (torchattacks.FAB, {"n_classes": 2, "eta": 10})
    FAB_eta20 = (torchattacks.FAB, {"n_classes": 2, "eta": 20})
    FAB_eta30 = (torchattacks.FAB, {"n_classes": 2, "eta": 30})

    # --- additive members for BASELINE.json's configurations ---
    PGD40_eps003 = (torchattacks.PGD, {"eps": 0.003, "steps": 40})          # configs 2 and 5 (alpha default 2/255)
    PGDL2_40 = (torchattacks.PGDL2, {"eps": 0.1, "steps": 40})             # config 3 (alpha default 0.2)
    CW = (torchattacks.CW, {"c": 1.0, "kappa": 0, "steps": 100, "lr": 0.01})  # config 4 (cw.py:27 advises c ~ 1)

    # --- additive members: APGD (step-size free), named like the PGD members above ---
    APGD = (torchattacks.APGD, {"norm": "Linf", "eps": 0.0005, "steps": 10})
    APGD_eps00075 = (torchattacks.APGD, {"norm": "Linf", "eps": 0.00075, "steps": 10})
    APGD_eps001 = (torchattacks.APGD, {"norm": "Linf", "eps": 0.001, "steps": 10})

    APGDL2 = (torchattacks.APGD, {"norm": "L2", "eps": 0.1, "steps": 10})
    APGDL2_eps15 = (torchattacks.APGD, {"norm": "L2", "eps": 0.15, "steps": 10})
    APGDL2_eps20 = (torchattacks.APGD, {"norm": "L2", "eps": 0.20, "steps": 10})

    APGD100_eps003 = (torchattacks.APGD, {"norm": "Linf", "eps": 0.003, "steps": 100})  # the standard budget at PGD40_eps003's radius

    # --- additive members: the momentum attacks made for transfer, named like the PGD members above; alpha = eps / steps, the
    # setting of the MI-FGSM paper (the classes' 2/255 default is 15x these radii and would fill the ball at the first step) ---
    MIFGSM = (torchattacks.MIFGSM, {"eps": 0.0005, "alpha": 0.0005 / 10, "steps": 10, "decay": 1.0})
    MIFGSM_eps00075 = (torchattacks.MIFGSM, {"eps": 0.00075, "alpha": 0.00075 / 10, "steps": 10, "decay": 1.0})
    MIFGSM_eps001 = (torchattacks.MIFGSM, {"eps": 0.001, "alpha": 0.001 / 10, "steps": 10, "decay": 1.0})

    NIFGSM = (torchattacks.NIFGSM, {"eps": 0.0005, "alpha": 0.0005 / 10, "steps": 10, "decay": 1.0})
    NIFGSM_eps00075 = (torchattacks.NIFGSM, {"eps": 0.00075, "alpha": 0.00075 / 10, "steps": 10, "decay": 1.0})
    NIFGSM_eps001 = (torchattacks.NIFGSM, {"eps": 0.001, "alpha": 0.001 / 10, "steps": 10, "decay": 1.0})

    VMIFGSM = (torchattacks.VMIFGSM, {"eps": 0.0005, "alpha": 0.0005 / 10, "steps": 10, "decay": 1.0, "N": 20, "beta": 1.5})
    VNIFGSM = (torchattacks.VNIFGSM, {"eps": 0.0005, "alpha": 0.0005 / 10, "steps": 10, "decay": 1.0, "N": 20, "beta": 1.5})

    MIFGSM40_eps003 = (torchattacks.MIFGSM, {"eps": 0.003, "alpha": 0.003 / 40, "steps": 40, "decay": 1.0})  # PGD40_eps003's radius

    # --- additive members: the worst case over the attacks of one threat model (torchattacks.MultiAttack: each member only on
    # the utterances the previous ones failed to flip).  The value's callable builds the members on the attacked model ---
    WORSTCASE = (torchattacks.MultiAttack.on_model, _worst_case_linf(0.0005))
    WORSTCASE_eps00075 = (torchattacks.MultiAttack.on_model, _worst_case_linf(0.00075))
    WORSTCASE_eps001 = (torchattacks.MultiAttack.on_model, _worst_case_linf(0.001))

    WORSTCASE_L2 = (torchattacks.MultiAttack.on_model, {"members": [("PGDL2", {"eps": 0.1, "steps": 10}),
                                                                    ("APGD", {"norm": "L2", "eps": 0.1, "steps": 10})]})

    WORSTCASE40_eps003 = (torchattacks.MultiAttack.on_model, _worst_case_linf(0.003, steps=40, apgd_steps=100))  # PGD40_eps003's radius

    # --- additive members: the radius at which each utterance breaks, in one run (torchattacks.MinRadiusPGD: a bisection per
    # utterance on [0, eps_max]); report_at = the radii of the PGD / PGDL2 triplets above, whose robust accuracies the run reports ---
    MINRADIUS = (torchattacks.MinRadiusPGD, {"norm": "Linf", "eps_max": 0.001, "search_steps": 6, "steps": 10,
                                             "report_at": (0.0005, 0.00075, 0.001)})
    MINRADIUS_L2 = (torchattacks.MinRadiusPGD, {"norm": "L2", "eps_max": 0.2, "search_steps": 6, "steps": 10,
                                                "report_at": (0.1, 0.15, 0.2)})
    MINRADIUS40_eps003 = (torchattacks.MinRadiusPGD, {"norm": "Linf", "eps_max": 0.003, "search_steps": 8, "steps": 40})  # PGD40_eps003's radius

    # --- additive members: the L1 threat model (torchattacks.APGDL1, l1-APGD).  eps_1 = 20 is a mean |delta| of 3.1e-4 over the
    # 64 600 samples of an utterance, the scale of L-inf 0.0005 and of L2 0.1 (RMS 3.9e-4): a choice of scale, not a measured
    # equivalence between the threat models ---
    APGDL1 = (torchattacks.APGDL1, {"eps": 20.0, "steps": 10})
    APGDL1_eps30 = (torchattacks.APGDL1, {"eps": 30.0, "steps": 10})
    APGDL1_eps40 = (torchattacks.APGDL1, {"eps": 40.0, "steps": 10})

    WORSTCASE_L1 = (torchattacks.MultiAttack.on_model, {"members": [("APGDL1", {"eps": 20.0, "steps": 10}),
                                                                    ("FAB", {"norm": "L1", "n_classes": 2, "eps": 20.0})]})

    # --- additive members: budgets in dB of waveform SNR (torchattacks.PGDSNR), per utterance (PGDSNR_*) or per 256-sample segment
    # (PGDSEGSNR_*).  40 / 30 / 20 dB are the customary figures of audio work (barely audible, audible, plainly noisy): a choice of
    # scale, not an equivalence to the `eps` members above, whose SNR differs by tens of dB from one utterance to the next ---
    PGDSNR_40dB = (torchattacks.PGDSNR, {"snr_db": 40.0, "segmental": False, "steps": 10})
    PGDSNR_30dB = (torchattacks.PGDSNR, {"snr_db": 30.0, "segmental": False, "steps": 10})
    PGDSNR_20dB = (torchattacks.PGDSNR, {"snr_db": 20.0, "segmental": False, "steps": 10})

    PGDSEGSNR_40dB = (torchattacks.PGDSNR, {"snr_db": 40.0, "segmental": True, "steps": 10})
    PGDSEGSNR_30dB = (torchattacks.PGDSNR, {"snr_db": 30.0, "segmental": True, "steps": 10})
    PGDSEGSNR_20dB = (torchattacks.PGDSNR, {"snr_db": 20.0, "segmental": True, "steps": 10})

    # --- additive members: one perturbation for every utterance (torchattacks.UniversalPGD), fitted on the first batches of the
    # run and applied to all of them (evaluation.generate_attacks: universal_fit / universal_load / universal_save).  The radii
    # are those of the PGD / PGDL2 members above; label 0 is spoof (base_dataset.py), so *_SPOOF is the noise an attacker adds
    # to any fake; UAP_WAVE_SPOOF's eps is 0.001 of full scale in the WAVEFORM's units, the same signal for every utterance.
    # All of these scales are choices, not measured equivalences ---
    UAP = (torchattacks.UniversalPGD, {"norm": "Linf", "eps": 0.0005})
    UAP_eps00075 = (torchattacks.UniversalPGD, {"norm": "Linf", "eps": 0.00075})
    UAP_eps001 = (torchattacks.UniversalPGD, {"norm": "Linf", "eps": 0.001})
    UAP_L2 = (torchattacks.UniversalPGD, {"norm": "L2", "eps": 0.1})
    UAP_SPOOF = (torchattacks.UniversalPGD, {"norm": "Linf", "eps": 0.0005, "source_label": 0})
    UAP_SPOOF_eps001 = (torchattacks.UniversalPGD, {"norm": "Linf", "eps": 0.001, "source_label": 0})
    UAP_WAVE_SPOOF = (torchattacks.UniversalPGD, {"norm": "Linf", "eps": 0.001, "source_label": 0, "domain": "waveform"})

    # --- additive members: one FIR filter for every fake (torchattacks.UniversalFilter, after Malafide: the convolutive threat
    # model), fitted and applied through the universal protocol above (universal_fit / universal_load / universal_save).  The
    # budget is the filter's length: 129 taps are 8 ms at 16 kHz, 257 are 16 ms, 1025 are 64 ms; label 0 is spoof.  The lengths,
    # lr = 0.02 and 5 epochs are choices of scale: nobody has measured what they achieve against a trained detector, and they are
    # not taken from the paper ---
    FILTER_SPOOF = (torchattacks.UniversalFilter, {"taps": 129, "source_label": 0})
    FILTER_SPOOF_L257 = (torchattacks.UniversalFilter, {"taps": 257, "source_label": 0})
    FILTER_SPOOF_L1025 = (torchattacks.UniversalFilter, {"taps": 1025, "source_label": 0})

    # --- additive members: the score-based black-box attack (torchattacks.SPSA: the attacker reads the detector's score and
    # takes no gradient), at the radii of the PGD triplet above.  20 steps of 8 direction pairs are 20 * 17 = 340 queries per
    # utterance, SPSA100_eps003 (PGD40_eps003's radius) 100 * 33 = 3300.  These budgets are choices of scale: nobody has
    # measured what they achieve against these detectors ---
    SPSA = (torchattacks.SPSA, {"eps": 0.0005, "steps": 20, "nb_sample": 8})
    SPSA_eps00075 = (torchattacks.SPSA, {"eps": 0.00075, "steps": 20, "nb_sample": 8})
    SPSA_eps001 = (torchattacks.SPSA, {"eps": 0.001, "steps": 20, "nb_sample": 8})
    SPSA100_eps003 = (torchattacks.SPSA, {"eps": 0.003, "steps": 100, "nb_sample": 16})

    # --- additive members: PGD on the gradient averaged over draws of a simulated audio channel (torchattacks.EOTPGD with
    # torchattacks.CHANNELS["mild"]), at the radii and 10 steps of the PGD triplet above, alpha = 2.5 * eps / steps, 4 draws per
    # step: 40 model passes per utterance, EOTPGD40_eps003 (PGD40_eps003's radius) 160.  These budgets and the channel are
    # choices of scale: nobody has measured what they achieve against these detectors or against a real device ---
    EOTPGD = (torchattacks.EOTPGD, {"eps": 0.0005, "alpha": 2.5 * 0.0005 / 10, "steps": 10, "eot_iter": 4, "channel": "mild"})
    EOTPGD_eps00075 = (torchattacks.EOTPGD, {"eps": 0.00075, "alpha": 2.5 * 0.00075 / 10, "steps": 10, "eot_iter": 4,
                                             "channel": "mild"})
    EOTPGD_eps001 = (torchattacks.EOTPGD, {"eps": 0.001, "alpha": 2.5 * 0.001 / 10, "steps": 10, "eot_iter": 4, "channel": "mild"})
    EOTPGD40_eps003 = (torchattacks.EOTPGD, {"eps": 0.003, "alpha": 2.5 * 0.003 / 40, "steps": 40, "eot_iter": 4,
                                             "channel": "mild"})    # budget unmeasured, as above

    # --- additive members: the sparse (L0) threat model (torchattacks.PGDL0: PGD0 of Croce & Hein, ICCV 2019): at most k samples
    # of an utterance change, each as far as [0, 1] allows - a handful of clicks.  k = 64 is about 0.1 % of a 64 600-sample
    # utterance; *_cap005 also bounds every change by 0.05 (the paper's "sparse and bounded" variant).  20 steps of
    # alpha = 0.15 per dimension, the paper's scale.  These budgets are choices of scale: nobody has measured what they achieve
    # against these detectors ---
    PGDL0 = (torchattacks.PGDL0, {"k": 64, "alpha": 0.15, "steps": 20})
    PGDL0_k256 = (torchattacks.PGDL0, {"k": 256, "alpha": 0.15, "steps": 20})
    PGDL0_k1024 = (torchattacks.PGDL0, {"k": 1024, "alpha": 0.15, "steps": 20})
    PGDL0_k1024_cap005 = (torchattacks.PGDL0, {"k": 1024, "alpha": 0.15, "steps": 20, "eps_inf": 0.05})

    # --- additive members: the label-only black-box attack (torchattacks.HopSkipJump: the attacker reads the detector's decision,
    # neither score nor gradient), at the radii of the PGD triplet above; report_at = those radii, whose robust accuracies the run
    # reports from the per-utterance radii.  10 iterations of 32 .. 101 probes, 4 candidate steps and 11 boundary searches of 12
    # rounds are at most 889 queries per utterance, HSJ50_eps003 (PGD40_eps003's radius) 16 089.  These budgets, delta_rel,
    # delta_min and search_steps are choices of scale: nobody has measured what they achieve against these detectors ---
    HSJ = (torchattacks.HopSkipJump, {"eps": 0.0005, "report_at": (0.0005, 0.00075, 0.001)})
    HSJ_eps00075 = (torchattacks.HopSkipJump, {"eps": 0.00075, "report_at": (0.0005, 0.00075, 0.001)})
    HSJ_eps001 = (torchattacks.HopSkipJump, {"eps": 0.001, "report_at": (0.0005, 0.00075, 0.001)})
    HSJ50_eps003 = (torchattacks.HopSkipJump, {"eps": 0.003, "steps": 50, "init_evals": 64, "max_evals": 1024})

    # --- additive members: PGD pulled under the psychoacoustic masking threshold of the clean utterance (torchattacks.PsyPGD: `steps`
    # of PGD inside the L-inf ball, then `mask_steps` that trade the classifier's gradient against the masking hinge's), at the
    # radii of PGD_eps001 and PGD40_eps003; alpha = eps / 10 (eps / 16 at 40 steps).  The budgets, alpha and mask_weight = 1 are
    # choices of scale: nobody has measured what they achieve against these detectors, or against listeners ---
    PSYPGD = (torchattacks.PsyPGD, {"eps": 0.001, "alpha": 0.001 / 10, "steps": 10, "mask_steps": 20, "mask_weight": 1.0})
    PSYPGD_eps003 = (torchattacks.PsyPGD, {"eps": 0.003, "alpha": 0.003 / 10, "steps": 10, "mask_steps": 20, "mask_weight": 1.0})
    PSYPGD40_eps003 = (torchattacks.PsyPGD, {"eps": 0.003, "alpha": 2.5 * 0.003 / 40, "steps": 40, "mask_steps": 40,
                                             "mask_weight": 1.0})    # budget unmeasured, as above

    # --- additive members: PGD on the SMOOTHED detector (torchattacks.SmoothAdvPGD: SmoothAdv of Salman et al., NeurIPS 2019 — the
    # soft vote over noisy copies of the iterate is differentiated, not the detector at one point), at the radii of the PGDL2
    # triplet above; alpha = 2 eps / steps.  sigma 0.05 in the waveform's units (with --certify the run's sigma replaces it), 8 noise
    # draws and 10 steps are 80 gradient passes per utterance.  sigma, the draws and the radii are choices of scale: nobody has
    # measured what they achieve against a detector trained under noise ---
    SMOOTHADV = (torchattacks.SmoothAdvPGD, {"eps": 0.1, "steps": 10, "sigma": 0.05, "samples": 8})
    SMOOTHADV_eps15 = (torchattacks.SmoothAdvPGD, {"eps": 0.15, "steps": 10, "sigma": 0.05, "samples": 8})
    SMOOTHADV_eps20 = (torchattacks.SmoothAdvPGD, {"eps": 0.20, "steps": 10, "sigma": 0.05, "samples": 8})

    # --- additive members: the minimal-norm attack (torchattacks.FMN: Fast Minimum-Norm of Pintor et al., NeurIPS 2021) — the radius
    # at which each utterance breaks as a continuous, uncapped figure: no eps_max, no outer search.  60 steps are the 60 gradient
    # passes MINRADIUS spends; report_at = the radii of the PGD / PGDL2 triplets above.  The schedules are the paper's defaults, a
    # choice of scale: nobody has measured what they achieve against a trained detector ---
    FMN = (torchattacks.FMN, {"norm": "Linf", "steps": 60, "report_at": (0.0005, 0.00075, 0.001)})
    FMN_L2 = (torchattacks.FMN, {"norm": "L2", "steps": 60, "report_at": (0.1, 0.15, 0.2)})
    FMN200 = (torchattacks.FMN, {"norm": "Linf", "steps": 200})

    # --- additive members: the sparse forms of the minimal-norm attack (torchattacks.FMNSparse) — the L1 norm and the number of changed
    # samples at which each utterance breaks, where APGDL1 and PGDL0 above only answer at fixed budgets; report_at = the radii of
    # the APGDL1 triplet and the budgets of the PGDL0 triplet.  The L0 member sets gamma_init itself: the paper's 0.05 grows an
    # integer radius by +1 per step (floor(1.05 eps) <= eps + 1 below eps = 20, and gamma is annealed while eps grows), so 100 steps
    # first meet 64 samples at step 63 and end at 101, short of 256 and 1024.  Steps, schedules and gamma_init = 0.3 are
    # choices of scale: nobody has measured what they achieve against a trained detector ---
    FMN_L1 = (torchattacks.FMNSparse, {"norm": "L1", "steps": 100, "report_at": (20.0, 30.0, 40.0)})
    FMN_L0 = (torchattacks.FMNSparse, {"norm": "L0", "steps": 100, "gamma_init": 0.3, "report_at": (64, 256, 1024)})

    NO_ATTACK = (None, {})
