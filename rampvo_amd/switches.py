"""The environment switches of the package, read in one place.

``read()`` parses them; the objects that use them call it when they are built (never at import) and keep the result as
instance attributes.  Nothing else in the package reads these variables (``_lib.LIB_PATH`` takes ``RAMP_HIP_LIB`` once,
when the library is loaded).  A value that does not parse, or is out of range, gives the default.

==========================  =======  ======================================================================================
variable                    default  meaning
==========================  =======  ======================================================================================
``RAMP_DEVICE_STEP``        1        anything but ``1``: every frame host driven (``Ramp_vo.device_steps``)
``RAMP_INPUTS_READY``       unset    ``1`` / ``stream``: ``Ramp_vo.inputs_ready`` defaults to True / ``"stream"``
``RAMP_NO_FLAG_WAITS``      0        non-zero: events, not signal words, order the tracker's streams
``RAMP_X3``                 1        anything but ``1``: the fp32 update operator on library GEMMs (``FusedUpdate.use_x3``)
``RAMP_CONV_X3``            1        ``0``: the fp32 towers on the exact-product f32 MFMA kernel (``encoder.conv_x3``)
``RAMP_CORR_F32_MFMA``      2        fp32 features: 2 split fp16 pairs, 1 fp32 MFMA, 0 reference order (``pack_f32``)
``RAMP_HOST_THREADS``       unset    ``0``: leave torch's host pool alone; ``n``: n threads (``hostenv.fit_host_threads``)
==========================  =======  ======================================================================================

Profilers and debug settings that make the runtime run one kernel at a time (``ROCPROF_COUNTER_COLLECTION``,
``AMD_SERIALIZE_KERNEL``, ``HIP_LAUNCH_BLOCKING``) switch the signal words off as ``RAMP_NO_FLAG_WAITS`` does: a wave
that waits for another stream's kernel needs the two to run concurrently.
"""
import dataclasses
import os


@dataclasses.dataclass(frozen=True)
class Switches:
    device_step: bool = True
    inputs_ready: object = False          # False, True or "stream"
    flag_waits: bool = True
    x3: bool = True
    conv_x3: bool = True
    corr_f32_mfma: int = 2
    host_threads: object = None           # None: the package's policy; 0: hands off; n > 0: n threads


def _on(env, name):
    return env.get(name, "0") not in ("", "0")


def read(env=None):
    """the switches as ``env`` (default: ``os.environ``) sets them"""
    env = os.environ if env is None else env
    try:
        corr = int(env.get("RAMP_CORR_F32_MFMA", "2"))
    except ValueError:
        corr = 2
    try:
        threads = int(env["RAMP_HOST_THREADS"]) if env.get("RAMP_HOST_THREADS", "") else None
    except ValueError:
        threads = None
    return Switches(
        device_step=env.get("RAMP_DEVICE_STEP", "1") == "1",
        inputs_ready={"stream": "stream", "1": True}.get(env.get("RAMP_INPUTS_READY", ""), False),
        flag_waits=not any(_on(env, k) for k in ("ROCPROF_COUNTER_COLLECTION", "AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING",
                                                 "RAMP_NO_FLAG_WAITS")),
        x3=env.get("RAMP_X3", "1") == "1",
        conv_x3=env.get("RAMP_CONV_X3", "1") != "0",
        corr_f32_mfma=corr if corr in (0, 1, 2) else 2,
        host_threads=threads if threads is None or threads >= 0 else None)
