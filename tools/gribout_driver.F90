! Driver of tools/make_golden_gribout.py: calls the reference's WGRIBENCODE_VALUES on the fields of a stream file and writes the vector VALUES it
! returns.  It is built by oracle/ref_build.py::build_driver: the routine, PARKIND_WAVE and YOWGRIBHD are the reference's own files, compiled
! unmodified in both precisions, behind the stand-ins of oracle/ref_stubs.F90 for what other packages supply.  Two modules are the driver's own,
! each the names the routine imports without using them on this path: YOWGRIB (the reference's is bound to the GRIB decoder) and OML_MOD (another
! package).  Built with -fopenmp: the routine declares OMP_GET_MAX_THREADS behind an OpenMP sentinel; its result does not depend on the number
! of threads (a maximum over chunks).
! Around the call the program restates the few statements of the callers that the routine takes for granted:
!   outspec.F90:96-118    the sea-ice mask  SPEC = (1 - ZMASK) FL1 + ZMASK FLMIN,  ZMASK = CICOVER > CITHRSH
!   outwspec.F90:124      FIELD(:,:) = ZMISS          (makegrid.F90:105-109 does the same)
!   outwspec.F90:222-226  IX = IXLG(IJ); IY = NGY - KXLT(IJ) + 1; FIELD(IX,IY) = block(IJ)      (makegrid.F90:156-160 does the same)
! Input  (stream, little endian): NGX, NGY, NPTS, IRGG, NTENCODE, NFLD, ITABPAR, ICE, LPADPOLES, NGRBRESS, ICHAR(CLDOMAIN) (int32);
!        AMONOP, AMOSOP, XDELLA, PPMISS, PPEPS, PPREC, PPRESOL, PPMIN_RESET, ZMISS, CITHRSH, FLMIN (real64); NLONRGG(NGY), IXLG(NPTS), KXLT(NPTS)
!        (int32); CICOVER(NPTS), BLOCK(NPTS,NFLD) (real64).  Every real is representable in the working precision.
! Output (stream): VALUES(NTENCODE) per field (real64): the working-precision result, widened.
MODULE YOWGRIB
  IMPLICIT NONE
  INTEGER, PARAMETER :: JPGRIB_SUCCESS = 0
  INTEGER :: IGRIB_GET_VALUE = 0, IGRIB_SET_VALUE = 0
END MODULE YOWGRIB

MODULE OML_MOD
  IMPLICIT NONE
  INTEGER :: OML_GET_MAX_THREADS = 1
END MODULE OML_MOD

PROGRAM GRIBOUT_DRIVER
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  USE YOWGRIBHD, ONLY : LLRSTGRIBPARAM
  IMPLICIT NONE
#include "wgribencode_values.intfb.h"

  INTEGER(KIND=JWIM) :: H(11), NGX, NGY, NPTS, IRGG, NTENCODE, NFLD, ITABPAR, ICE, NGRBRESS, IJ, IX, IY, IFLD
  LOGICAL :: LPADPOLES
  CHARACTER(LEN=1) :: CLDOMAIN
  REAL(KIND=8) :: R(11)
  REAL(KIND=JWRB) :: AMONOP, AMOSOP, XDELLA, PPMISS, PPEPS, PPREC, PPRESOL, PPMIN_RESET, ZMISS, CITHRSH, FLMIN
  INTEGER(KIND=JWIM), ALLOCATABLE :: NLONRGG(:), IXLG(:), KXLT(:)
  REAL(KIND=8), ALLOCATABLE :: CI8(:), B8(:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: ZMASK(:), SPEC(:), FIELD(:,:), VALUES(:)
  CHARACTER(LEN=512) :: FIN, FOUT

  LLRSTGRIBPARAM = .FALSE.
  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  OPEN(11, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(12, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  READ(11) H, R
  NGX = H(1); NGY = H(2); NPTS = H(3); IRGG = H(4); NTENCODE = H(5); NFLD = H(6); ITABPAR = H(7); ICE = H(8); LPADPOLES = H(9) /= 0
  NGRBRESS = H(10); CLDOMAIN = ACHAR(H(11))
  AMONOP = REAL(R(1), JWRB); AMOSOP = REAL(R(2), JWRB); XDELLA = REAL(R(3), JWRB); PPMISS = REAL(R(4), JWRB); PPEPS = REAL(R(5), JWRB)
  PPREC = REAL(R(6), JWRB); PPRESOL = REAL(R(7), JWRB); PPMIN_RESET = REAL(R(8), JWRB); ZMISS = REAL(R(9), JWRB); CITHRSH = REAL(R(10), JWRB)
  FLMIN = REAL(R(11), JWRB)
  ALLOCATE(NLONRGG(NGY), IXLG(NPTS), KXLT(NPTS), CI8(NPTS), B8(NPTS,NFLD), ZMASK(NPTS), SPEC(NPTS), FIELD(NGX,NGY), VALUES(NTENCODE))
  READ(11) NLONRGG, IXLG, KXLT, CI8, B8

  DO IJ = 1, NPTS
    IF (REAL(CI8(IJ), JWRB) > CITHRSH) THEN
      ZMASK(IJ) = 1.0_JWRB
    ELSE
      ZMASK(IJ) = 0.0_JWRB
    ENDIF
  ENDDO

  DO IFLD = 1, NFLD
    IF (ICE /= 0) THEN
      SPEC(:) = (1.0_JWRB - ZMASK(:)) * REAL(B8(:,IFLD), JWRB) + ZMASK(:)*FLMIN
    ELSE
      SPEC(:) = REAL(B8(:,IFLD), JWRB)
    ENDIF
    FIELD(:,:) = ZMISS
    DO IJ = 1, NPTS
      IX = IXLG(IJ)
      IY = NGY - KXLT(IJ) + 1
      FIELD(IX,IY) = SPEC(IJ)
    ENDDO
    VALUES(:) = 0.0_JWRB
    CALL WGRIBENCODE_VALUES(NGX, NGY, FIELD, ITABPAR, .FALSE., PPMISS, PPEPS, PPREC, PPRESOL, PPMIN_RESET, NTENCODE, NGRBRESS, LPADPOLES, &
 &                          NGY, NLONRGG, IRGG, AMONOP, AMOSOP, XDELLA, CLDOMAIN, ZMISS, VALUES)
    WRITE(12) REAL(VALUES, 8)
  ENDDO
  CLOSE(11)
  CLOSE(12)
END PROGRAM GRIBOUT_DRIVER
