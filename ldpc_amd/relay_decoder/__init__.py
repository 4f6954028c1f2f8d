"""``ldpc_amd.relay_decoder`` -- Relay-BP on MI355X (no counterpart in the reference): chained memory min-sum legs decoded in one call
(``ldpc_hip_bp_set_relay``)."""
from ldpc_amd.relay_decoder._relay_decoder import RelayBpDecoder, relay_schedule

__all__ = ["RelayBpDecoder", "relay_schedule"]
