"""StepOperands: the A_t, B_t, C_t, Q_t one filter pass used, in whichever of the two forms lgssm_ops takes them - slots of ONE
packed step record (mix_dynamics, the in-kernel alpha-LSTM) or plain stacks ([r,c] shared, [B,T,r,c] per step).  KalmanFilter
keeps the bundle of its latest pass so that the read-outs and the ELBO which are handed that pass's A_list / B_list / C_list back
(the reference API) reach the record again instead of the strided views; which form a pass produced is known here only.
"""
from typing import NamedTuple, Optional

import torch

from .lgssm_ops import Slots


class StepOperands(NamedTuple):
    views: tuple                            # (A_list, B_list, C_list) [B,T,r,c], what the reference API returns
    record: Optional[torch.Tensor] = None   # packed step record [B,T,E]
    slots: Slots = Slots()                  # where the record holds A | B | C | Q; an operand without a slot is plain:
    A: Optional[torch.Tensor] = None
    B: Optional[torch.Tensor] = None
    C: Optional[torch.Tensor] = None
    Q: Optional[torch.Tensor] = None
    Q_view: Optional[torch.Tensor] = None   # [B,T,n,n] view of the record's Q slot

    @classmethod
    def packed(cls, record, slots, views, C=None, Q=None, Q_view=None):
        """A step record with its slots; C / Q plain where the record has no slot for them (Q_view where it has one for Q)."""
        return cls(tuple(views), record, slots, C=C, Q=Q, Q_view=Q_view)

    @classmethod
    def plain(cls, A, B, C, Q, views=None):
        """Plain stacks; `views` only where A, B, C are shared [r,c] matrices and the views their [B,T,r,c] expansions."""
        return cls((A, B, C) if views is None else tuple(views), A=A, B=B, C=C, Q=Q)

    def owns(self, A_list, B_list, C_list):
        """Are these the very tensors this pass returned (identity: equal values from another pass do not count)."""
        return all(a is b for a, b in zip((A_list, B_list, C_list), self.views))

    def emission(self, C_list=None):
        """(Cm, packed, Slots(C=...)) as lgssm_ops' read-outs take C_t.  A C_list that is not this pass's own comes back as the
        plain stack it is."""
        if C_list is not None and C_list is not self.views[2]:
            return C_list, None, Slots()
        return self.C if self.C is not None else self.views[2], self.record, Slots(C=self.slots.C)

    def transition_noise(self):
        """Q_t as a tensor: [n,n] or [B,T,n,n] (the view of the Q slot where Q is packed)."""
        return self.Q if self.Q is not None else self.Q_view

    def posterior(self):
        """(A, Cm, Q, packed, slots) of lgssm_ops.posterior_paths."""
        Cm, packed, _ = self.emission()
        return self.views[0], Cm, self.transition_noise(), packed, self.slots._replace(B=None)

    def lgssm(self, R, mu0, Sigma0):
        """The operand arguments of LgssmSmooth / LgssmElbo, `packed` through `slots`."""
        return self.record, self.A, self.B, self.C, self.Q, R, mu0, Sigma0, self.slots


NO_PASS = StepOperands.plain(None, None, None, None)   # before the first pass: owns nothing
