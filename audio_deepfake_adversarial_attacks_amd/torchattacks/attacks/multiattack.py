"""MultiAttack (reference: adversarial_attacks/torchattacks/attacks/multiattack.py:7-133)."""
import contextlib

import torch

from ..attack import Attack


class MultiAttack(Attack):
    r"""MultiAttack runs a list of attacks on the same utterances and labels: each member only on the rows the previous ones
    failed to flip.  The first successful adversarial row per utterance is kept; rows no member flips come back unchanged.

    Arguments:
        attacks (list): list of attacks, all on the same model.
        verbose (bool): print the success rate after every member at each call. (Default: False)

    Adaptations to (B, T) waveform detectors with one logit: success is judged on cat([-z, z], 1), i.e. the prediction is
    z > 0 (the reference's `torch.max(outputs, 1)` on a (B, 1) logit is always class 0), with the model in eval mode; a
    stage's whole bookkeeping (multiattack.py:55-66) is one fused call (hip_ops.multi_route) and one host read of its two
    counters.  Members called on fewer rows than the incoming batch never capture a hipGraph (torchattacks/graphed.py).

    Examples::
        >>> atk1 = torchattacks.PGD(model, eps=0.001, steps=10)
        >>> atk2 = torchattacks.APGD(model, norm="Linf", eps=0.001, steps=10)
        >>> attack = torchattacks.MultiAttack([atk1, atk2])
        >>> adv_images = attack(images, labels)
    """

    replays_from_graph = False      # a host read per stage: evaluation.generate_attacks keeps one batch in flight

    def __init__(self, attacks, verbose=False):
        # multiattack.py:24-39
        if len(attacks) == 0:
            raise ValueError("At least one attack should be provided.")
        if len({id(attack.model) for attack in attacks}) != 1:
            raise ValueError("At least one of attacks is referencing a different model.")

        super().__init__("MultiAttack", attacks[0].model)
        self.attacks = attacks
        self.verbose = verbose
        self._accumulate_multi_atk_records = False
        self._multi_atk_records = [0.0]
        self._supported_mode = ["default"]

    @classmethod
    def on_model(cls, model, members, verbose=False):
        """MultiAttack over `members` = [(attack class name, kwargs), ...], each built on `model`: the form an AttackEnum
        value (callable, kwargs) needs for `attack_method(attack_model, **attack_params)`."""
        from ... import torchattacks
        attacks = [getattr(torchattacks, name)(model, **kwargs) for name, kwargs in members]
        for attack in attacks:
            if getattr(attack, "wants_minmax", False):
                raise ValueError(f"{attack.attack} needs each utterance's min and max (set_minmax), which MultiAttack's row "
                                 "compaction does not route to its members: it cannot be a member")
        return cls(attacks, verbose=verbose)

    def set_training_mode(self, model_training=False, batchnorm_training=False, dropout_training=False):
        """Also forwarded to the members: they switch the model themselves at every call (Attack.__call__), and the evaluation
        loop sets the mode on the outer object only."""
        super().set_training_mode(model_training, batchnorm_training, dropout_training)
        for attack in self.attacks:
            attack.set_training_mode(model_training, batchnorm_training, dropout_training)

    @staticmethod
    @contextlib.contextmanager
    def _eager(attack, on):
        """graphed.run_iterations' per-attack off switch, set for the duration of one member call."""
        before = attack._graph_off
        attack._graph_off = before or on
        try:
            yield
        finally:
            attack._graph_off = before

    def forward(self, images, labels):
        r"""
        Overridden.
        """
        ops = self.ops
        images, labels, _ = self._prepare(images, labels)
        batch_size = images.shape[0]
        final_images = images.clone()
        rows = torch.arange(batch_size, dtype=torch.int32, device=images.device)
        x, y, n = images, labels.to(torch.int64), batch_size

        multi_atk_records = [batch_size]

        for attack in self.attacks:
            # a survivor count is not a workload: a capture per count would evict the full-batch captures (graphed._MAX_GRAPHS)
            with self._eager(attack, n < batch_size):
                adv_images = attack(x, y)

            # judged by the detector as it is deployed: a member's call may leave the model's layers in their training modes
            self.model.eval()
            with torch.no_grad():
                z = self.model(adv_images)
            if z.dim() != 2 or z.shape[1] != 1:
                raise ValueError(f"the attacked model must emit one logit per utterance, got {tuple(z.shape)}")

            # multiattack.py:55-66: wrong rows to final_images, the others compacted for the next member
            x, y, rows, counts = ops.multi_route(adv_images.detach().contiguous(), x, z.detach().reshape(-1).contiguous(), y,
                                                 rows, final_images)
            n = int(counts[1])                                   # the stage's only host read
            x, y, rows = x[:n], y[:n], rows[:n]
            multi_atk_records.append(n)

            if n == 0:
                break

        if self.verbose:
            print(self._return_sr_record(multi_atk_records))

        if self._accumulate_multi_atk_records:
            self._update_multi_atk_records(multi_atk_records)

        return final_images

    # ---- records (multiattack.py:80-93) ------------------------------------------------------------------------------------

    def _clear_multi_atk_records(self):
        self._multi_atk_records = [0.0]

    def _covert_to_success_rates(self, multi_atk_records):
        sr = [((1 - multi_atk_records[i] / multi_atk_records[0]) * 100) for i in range(1, len(multi_atk_records))]
        return sr

    def _return_sr_record(self, multi_atk_records):
        sr = self._covert_to_success_rates(multi_atk_records)
        return "Attack success rate: " + " | ".join(["%2.2f %%" % item for item in sr])

    def _update_multi_atk_records(self, multi_atk_records):
        for i, item in enumerate(multi_atk_records):
            self._multi_atk_records[i] += item

    def _start_multi_atk_records(self):
        """multiattack.py:99-105: one accumulator per member after the batch-size slot; calls add to them until cleared."""
        self._clear_multi_atk_records()
        self._accumulate_multi_atk_records = True
        self._multi_atk_records.extend(0.0 for _ in self.attacks)

    def save(self, data_loader, save_path=None, verbose=True, return_verbose=False, save_pred=False):
        r"""
        Overridden.
        """
        # multiattack.py:95-125
        prev_verbose = self.verbose
        self.verbose = False
        self._start_multi_atk_records()

        if return_verbose:
            rob_acc, l2, elapsed_time = super().save(data_loader, save_path, verbose, return_verbose, save_pred=save_pred)
            sr = self._covert_to_success_rates(self._multi_atk_records)
        elif verbose:
            super().save(data_loader, save_path, verbose, return_verbose, save_pred=save_pred)
        else:
            super().save(data_loader, save_path, verbose=False, return_verbose=False, save_pred=save_pred)

        self._clear_multi_atk_records()
        self._accumulate_multi_atk_records = False
        self.verbose = prev_verbose

        if return_verbose:
            return rob_acc, sr, l2, elapsed_time

    def _save_print(self, progress, rob_acc, l2, elapsed_time, end):
        r"""
        Overridden.
        """
        print("- Save progress: %2.2f %% / Robust accuracy: %2.2f %%" % (progress, rob_acc)
              + " / " + self._return_sr_record(self._multi_atk_records)
              + " / L2: %1.5f (%2.3f it/s) \t" % (l2, elapsed_time), end=end)
