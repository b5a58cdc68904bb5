"""Python harness over the C ABI of the MI355X flow engine (include/aof.h).

The product is ``csrc/libaof.so`` (hand-written gfx950 kernels behind a plain C
ABI) and the C++ facade in ``facade/``; this package only binds the C ABI with
``ctypes`` so that tests and ``bench.py`` can drive it with device memory owned
by PyTorch.  It mirrors the reference's operator surface for the path --
``OpticalFlowPX4.calcFlow`` as called from
``/root/reference/src/mainloop.cpp:322`` -- in :class:`OpticalFlowPX4`.

A module per concern, re-exported here: ``_abi`` (include/aof.h restated, and ``lib``), ``_util`` (shared helpers),
``engine`` (parameters, batch, field, sequence, ``FlowEngine``), ``bank`` (the stream bank), ``facade`` (the second library).

There is no CPU fallback anywhere in this package: if ``libaof.so`` is missing
the import raises, and every compute entry point needs a gfx950 device.

The directory name contains a hyphen, so import it through
``__graft_entry__.load_package()`` (registers it as ``aero_optical_flow_amd``).
"""
from __future__ import annotations

from ._abi import *   # noqa: F401,F403 -- the header: every constant, record, dtype, AofError, lib, EXPORTS, LIB_PATH
from ._abi import _HERE, _load   # noqa: F401
from .engine import (FlowEngine, abs_diffs, algorithmic_bytes, blocks_view, check_params, default_params,  # noqa: F401
                     derotate_batch, exposure_msv, field_host, field_params, field_supported, fields_view, flow_angle,
                     flows_view, grid, ingest_batch, px4flow_params, sequence_layout, sequence_params, workspace_layout)
from .bank import (Bank, HostOutbox, _aligned_copy, _sensor_record, bank_burst_params, bank_camera_layout,  # noqa: F401
                   bank_camera_params, bank_imu_host, bank_layout, bank_mavlink_rx_host, bank_params,
                   bank_pixel_row_bytes, bank_sensor_centred, bank_sensor_from_camera, bank_sensor_valid,
                   bank_stream_from_params, bank_warp_crossover, bank_warp_one_launch, exposure_commands_view,
                   exposure_control_default, exposure_control_host, exposure_states_view, exposure_view, imu_params,
                   imu_states_view, ingest_sensors, ingest_warped, mavlink_rx_params, mavlink_rx_states_view,
                   outbox_layout, outbox_view, ticks_view, warp_host, warp_mesh_from_lens, warp_mesh_identity,
                   warp_mesh_size)
from .facade import (DEFAULT_FLOW_FEATURE_THRESHOLD, DEFAULT_FLOW_VALUE_THRESHOLD, DEFAULT_IMAGE_HEIGHT,  # noqa: F401
                     DEFAULT_IMAGE_WIDTH, DEFAULT_OUTPUT_RATE, DEFAULT_SEARCH_SIZE, FACADE_PATH, OpticalFlowBank,
                     OpticalFlowOpenCV, OpticalFlowPX4, _FacadeFlow, _facade, facade_lib, pack_optical_flow_rad)
