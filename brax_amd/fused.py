"""The `fused` switch every kernel entry point takes, in one place.

False: the chained form, and the support check is not run. True: the kernel,
or `NotImplementedError('no fused <what>: <why>')`. None: the kernel where it
applies, else the chained form.
"""
from typing import Callable, Optional


def use_kernel(fused: Optional[bool], what: str, why_not: Callable[[], Optional[str]]) -> bool:
  """Whether a call with this `fused` takes the kernel. `why_not()` is the
  site's support check: None when the kernel applies, else the reason."""
  if fused is False:
    return False
  why = why_not()
  if why is None:
    return True
  if fused is True:
    raise NotImplementedError(f'no fused {what}: {why}')
  return False
