"""Every kernel gfx950 compiles from gym.net_amd/csrc/rollout_inputs.hip, and the gymnet_rollout_inputs_device arguments that reach it — a
restatement of pick_rollout_inputs_form (rollout_inputs.hpp): four floats per thread (16-byte stores) need history * obs_dim % 4 == 0,
x_row_stride % 4 == 0 and a 16-byte aligned d_x, whatever the lane count (there is no lane-count threshold) and whatever the inputs'
alignment; dense or gathered is whether d_rows is given; float64 is obs_f64.  The kernel that writes d_history_out runs beside either.
tests/test_rollout_inputs_host.py holds the table to the compiled set; tests/test_gpu_rollout_inputs.py launches every row."""

BLOCK = 256
MIN_ROWS = 8                  # rollout_inputs.hpp kRolloutInputsMinRows
TARGET_THREADS = 32 * 64 * 1024
ROWS_IN_FLIGHT = 4            # rollout_inputs.hip kRowsInFlight


def _b(x):
    return "true" if x else "false"


def row_kernel(vec, f64, gathered):
    return f"rollout_inputs_{'gather' if gathered else 'dense'}_kernel<{vec},{_b(f64)}>"


def history_kernel(f64):
    return f"rollout_inputs_history_kernel<{_b(f64)}>"


def vec_for(width, x_row_stride, x_ptr):
    return 4 if width % 4 == 0 and x_row_stride % 4 == 0 and x_ptr % 16 == 0 else 1


def kernels_for(obs_dim, history, x_row_stride, x_ptr, f64, gathered, history_out):
    """the kernels a call with rows to write launches, by name"""
    out = {row_kernel(vec_for(obs_dim * history, x_row_stride, x_ptr), f64, gathered)}
    if history_out:
        out.add(history_kernel(f64))
    return out


def chunks_for(steps, count, obs_dim, history, vec, target=TARGET_THREADS):
    """(rows_per_chunk, chunks) of the dense form"""
    cols = count * (obs_dim * history // vec)
    per_chunk = -(-cols // BLOCK) * BLOCK
    want = -(-target // per_chunk) if target > per_chunk else 1
    r = min(steps, max(-(-steps // want), max(history, MIN_ROWS)))
    return r, -(-steps // r)


FORMS = [{"kernel": row_kernel(vec, f64, gathered), "vec": vec, "f64": f64, "gathered": gathered,
          # obs_dim, history, x_row_stride - width, d_x offset in floats: arguments that reach the row at any lane count
          "reach": {"obs_dim": 4, "history": 4, "pad": 0 if vec == 4 else 3, "offset": 0}}
         for vec in (1, 4) for f64 in (False, True) for gathered in (False, True)]
HISTORY_KERNELS = [history_kernel(False), history_kernel(True)]
