"""xtddft_amd -- MI355X-native TDA response hot path of XTDDFT.

Reference-compatible entry points (PySCF-style operator API):

* ``XTDA(mol, mf, ...)``                (xtddft/XTDA.py)
* ``SF_TDA(mf, isf, davidson, method)`` (xtddft/SF_TDA.py) and
  ``gen_tda_operation_sf``, ``init_guess``, ``davidson_process``
* ``XSF_TDA(mf, SA, ...)``              (xtddft/XSF_TDA.py)
* ``davidson1``                         (xtddft/utils/Davidson.py)
* ``OSsTDA(mol, mf, ...)``              (xtddft/sTDA/os_sTDA.py)
* ``SI_driver(mf, S, Vso, ...)``        (x2c_hamiltonian/driver/si_driver.py) and the
  ``states_from_xsf`` / ``states_from_xtda`` / ``states_from_sf_up`` helpers
* ``SF_TDA_down(mf).nuc_grad_method()`` / ``SF_TDA_up(mf).nuc_grad_method()`` and
  ``qc.UHF(mol).nuc_grad_method()``     (xtddft/grad_jp/grad/usfcis.py; ``xtddft_amd/grad.py``)
* ``qc.UKS(mol, xc).to_device().nuc_grad_method()``: the UKS ground-state gradient, LDA / GGA,
  pure and global hybrid (the mean-field gradient xtddft/grad_hb/tduks_sfu.py starts from;
  ``xtddft_amd/qc/grad.py`` ``KSGradients``)
* ``SFU_gradient(td, method=1, state=1)`` / ``SFD_gradient(td, method=1, state=1)``: spin-flip TDA
  gradients on a UKS reference with the multicollinear (1) or collinear (2) kernel
  (xtddft/grad_hb/tduks_sfu.py; ``xtddft_amd/grad.py``)
* ``XTDA(mol, mf).nuc_grad_method()``: U-TDA gradients on a UHF / UKS reference, LDA / GGA, pure and
  global hybrid (xtddft/grad_jp/grad/utdhf.py with Y = 0; ``xtddft_amd/grad_utda.py``)

The arithmetic runs in the HIP library ``_lib/libxtddft_amd.so`` (C ABI in
``include/xtddft_amd.h``); there is no CPU fallback.
"""
from .meanfield import Grid, MeanField, Mole
from .utils import HA2EV, HA2EV_XSF, order_pyscf2my, so2st, st2so

__all__ = ["Grid", "MeanField", "Mole", "HA2EV", "HA2EV_XSF", "order_pyscf2my", "so2st", "st2so",
           "XTDA", "SF_TDA", "SF_TDA_up", "SF_TDA_down", "XSF_TDA", "davidson1", "DeviceOperator", "OSsTDA",
           "SI_driver", "si_couple", "states_from_xsf", "states_from_xtda", "states_from_sf_up",
           "get_soDKH1_somf", "vso_mo", "SFU_gradient", "SFD_gradient"]


def __getattr__(name):   # lazy: importing the package must not require a GPU
    if name == "XTDA":
        from .xtda import XTDA
        return XTDA
    if name in ("SF_TDA", "SF_TDA_up", "SF_TDA_down"):
        from . import sf_tda
        return getattr(sf_tda, name)
    if name == "XSF_TDA":
        from .xsf_tda import XSF_TDA
        return XSF_TDA
    if name == "davidson1":
        from .davidson import davidson1
        return davidson1
    if name == "OSsTDA":
        from .stda import OSsTDA
        return OSsTDA
    if name in ("SI_driver", "si_couple", "states_from_xsf", "states_from_xtda", "states_from_sf_up"):
        from . import soc
        return getattr(soc, name)
    if name in ("get_soDKH1_somf", "vso_mo"):
        from . import somf
        return getattr(somf, name)
    if name in ("SFU_gradient", "SFD_gradient"):
        from . import grad
        return getattr(grad, name)
    if name == "DeviceOperator":
        from .operator import DeviceOperator
        return DeviceOperator
    raise AttributeError(name)
