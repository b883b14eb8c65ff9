"""Mirror of the reference's ``openpoints.utils``: the checkpoint functions of its training loop (ckpt_util.py)."""
from .ckpt_util import load_checkpoint, resume_checkpoint, save_checkpoint  # noqa: F401
