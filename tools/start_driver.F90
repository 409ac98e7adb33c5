! Driver of tools/make_golden_start.py: calls the reference's MSTART (with PEAK, SPECTRA, JONSWAP, SPR), UNSETICE and SDEPTHLIM (with SEMEAN) on
! the records of a stream file and writes what they return.  It is built by oracle/ref_build.py::build_driver: the routines and the modules
! they use are the reference's own files, compiled unmodified in both precisions, behind the stand-ins of oracle/ref_stubs.F90 for what other
! packages supply; the driver holds no module of its own.  The program fills the modules' variables from the file, so that the reference sees
! the tables of ecwam_amd/tables.py, the ones the device holds, and compares what the reference declares a PARAMETER (EPSMIN, WETAIL, FLMIN).
! For the tail of GETSPEC the program restates the fill loop of getspec.F90:650-656 -- three lines inside a routine that reads GRIB files --
! and calls the reference's SDEPTHLIM, as getspec.F90:658 does.
! Input  (stream, little endian): NPTS, NANG, NFRE (int32); FR(NFRE), TH(NANG), DFIM(NFRE), FR5(NFRE), then G, PI, ZPI, ZPI4GM2, EPSMIN, DELTH,
!        WETAIL, FLMIN (real64); then records, each led by an int32:
!          1 MSTART:   IOPTI (int32); FETCH, FRMAX, THETAQ, FM, ALFA, ZGAMMA, SA, SB (real64); WSWAVE(NPTS), WDWAVE(NPTS)
!          2 UNSETICE: LICERUN, LMASKICE, LBIWBK (int32); CITHRSH, DELPHI (real64); DEPTH, EMAXDPT, WDWAVE, WSWAVE, CICOVER (NPTS each);
!                      FL1(NPTS,NANG,NFRE)
!          3 the tail: NFRE_RED (int32); EMAXDPT(NPTS); FL1(NPTS,NANG,NFRE)
!          0 the end
!        Every real is representable in the working precision.
! Output (stream): per record FL1(NPTS,NANG,NFRE) (real64): the working-precision result, widened.
PROGRAM START_DRIVER
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  USE YOWPARAM, ONLY : NANG, NFRE
  USE YOWPCONS, ONLY : G, PI, ZPI, ZPI4GM2, EPSMIN, DEG, R
  USE YOWFRED, ONLY : FR, TH, DFIM, FR5, FRM5, DELTH, WETAIL
  USE YOWSTAT, ONLY : LBIWBK
  USE YOWGRID, ONLY : DELPHI
  USE YOWICE, ONLY : FLMIN, CITHRSH, LICERUN, LMASKICE
  USE YOWMAP, ONLY : CLDOMAIN
  USE YOWTEXT, ONLY : LRESTARTED
  IMPLICIT NONE
  INTEGER, PARAMETER :: R8 = SELECTED_REAL_KIND(13, 300)
  INTEGER(KIND=JWIM) :: NPTS, OP, IOPTI, L1, L2, L3, NFRE_RED, M
  REAL(KIND=R8) :: S(8)
  REAL(KIND=R8), ALLOCATABLE :: A8(:), F8(:,:,:), P8(:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: FL1(:,:,:), P(:,:)
  CHARACTER(LEN=512) :: FIN, FOUT

  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  OPEN(11, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(12, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  READ(11) NPTS, NANG, NFRE
  ALLOCATE(FR(NFRE), TH(NANG), DFIM(NFRE), FR5(NFRE), FRM5(NFRE), F8(NPTS,NANG,NFRE), FL1(NPTS,NANG,NFRE), P8(NPTS,5), P(NPTS,5))
  ALLOCATE(A8(NFRE))
  READ(11) A8
  FR = REAL(A8, JWRB)
  DEALLOCATE(A8)
  ALLOCATE(A8(NANG))
  READ(11) A8
  TH = REAL(A8, JWRB)
  DEALLOCATE(A8)
  ALLOCATE(A8(NFRE))
  READ(11) A8
  DFIM = REAL(A8, JWRB)
  READ(11) A8
  FR5 = REAL(A8, JWRB)
  FRM5 = 1.0_JWRB/FR5          ! initmdl.F90:466
  READ(11) S
  G = REAL(S(1), JWRB)
  PI = REAL(S(2), JWRB)
  ZPI = REAL(S(3), JWRB)
  ZPI4GM2 = REAL(S(4), JWRB)
  IF (REAL(S(5), JWRB) /= EPSMIN) ERROR STOP 'EPSMIN'
  DELTH = REAL(S(6), JWRB)
  IF (REAL(S(7), JWRB) /= WETAIL) ERROR STOP 'WETAIL'
  IF (REAL(S(8), JWRB) /= FLMIN) ERROR STOP 'FLMIN'
  DEG = 180.0_JWRB/PI
  R = 0.0_JWRB
  CLDOMAIN = 'g'
  LRESTARTED = .FALSE.
  DO
    READ(11) OP
    IF (OP == 0) EXIT
    IF (OP == 1) THEN
      READ(11) IOPTI, S, P8(:,1:2)
      P = REAL(P8, JWRB)
      CALL MSTART(IOPTI, REAL(S(1), JWRB), REAL(S(2), JWRB), REAL(S(3), JWRB), REAL(S(4), JWRB), REAL(S(5), JWRB), REAL(S(6), JWRB),  &
 &                REAL(S(7), JWRB), REAL(S(8), JWRB), 1_JWIM, NPTS, FL1, P(:,1), P(:,2))
    ELSEIF (OP == 2) THEN
      READ(11) L1, L2, L3, S(1:2), P8, F8
      LICERUN = L1 /= 0
      LMASKICE = L2 /= 0
      LBIWBK = L3 /= 0
      CITHRSH = REAL(S(1), JWRB)
      DELPHI = REAL(S(2), JWRB)
      P = REAL(P8, JWRB)
      FL1 = REAL(F8, JWRB)
      CALL UNSETICE(1_JWIM, NPTS, P(:,1), P(:,2), P(:,3), P(:,4), P(:,5), FL1)
    ELSE
      READ(11) NFRE_RED, P8(:,1), F8
      P = REAL(P8, JWRB)
      FL1 = REAL(F8, JWRB)
      DO M = NFRE_RED + 1, NFRE      ! every bin above NFRE_RED: the last one read, times FR5 there, times FRM5 here (in that order)
        FL1(:,:,M) = (FL1(:,:,NFRE_RED) * FR5(NFRE_RED)) * FRM5(M)
      ENDDO
      CALL SDEPTHLIM(1_JWIM, NPTS, P(:,1), FL1)
    ENDIF
    WRITE(12) REAL(FL1, R8)
  ENDDO
  CLOSE(11)
  CLOSE(12)
END PROGRAM START_DRIVER
